"""ctypes binding of the C ABI in include/xalm_hip.h (libxalm_hip.so, built in-tree).

There is no fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
# XALM_HIP_LIB: another build of the same library (launch-structure experiments, tools/)
HIP_LIB_PATH = os.environ.get("XALM_HIP_LIB") or os.path.join(LIB_DIR, "libxalm_hip.so")

# enum xh_dtype (the reference's Type ids, src/types.h:505-514)
F32, F16, BF16, F8_E4M3, F8_E5M2, U8, Q8 = 1, 2, 3, 6, 7, 8, 9
# the converter's gguf blocks (convert.py:176-187, quants.py): this build's ids
Q8_0, Q4_0, Q4_1, Q5_0, Q5_1 = 20, 21, 22, 23, 24
# OCP microscaling FP4: 32 e2m1 codes under one E8M0 scale byte (include/xalm_hip.h)
MXFP4 = 25
# gguf K-quants: super-blocks of 256 elements (include/xalm_hip.h)
Q4_K, Q6_K = 26, 27
DTYPE_BY_NAME = {"F32": F32, "F16": F16, "BF16": BF16, "F8_E4M3": F8_E4M3, "F8_E5M2": F8_E5M2,
                 "U8": U8, "Q8": Q8, "Q8_0": Q8_0, "Q4_0": Q4_0, "Q4_1": Q4_1, "Q5_0": Q5_0, "Q5_1": Q5_1,
                 "MXFP4": MXFP4, "Q4_K": Q4_K, "Q6_K": Q6_K}
DTYPE_SIZE = {F32: 4, F16: 2, BF16: 2, F8_E4M3: 1, F8_E5M2: 1, U8: 1, Q8: 1}
# bytes per 32-element block: f16 d, [f16 m], [u32 qh], codes (quants.py); MXFP4: e, codes
GQ_BLOCK_BYTES = {Q8_0: 34, Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, MXFP4: 17}
# bytes per 256-element super-block of the K-quants
KQ_BLOCK_BYTES = {Q4_K: 144, Q6_K: 210}


def block_geometry(dtype: int):
    """(elements, bytes) of one block of a block dtype in the file layout, None for any other."""
    if dtype in GQ_BLOCK_BYTES:
        return 32, GQ_BLOCK_BYTES[dtype]
    if dtype in KQ_BLOCK_BYTES:
        return 256, KQ_BLOCK_BYTES[dtype]
    return None


def row_bytes(dtype: int, n: int) -> int:
    """Bytes of one n-element row as uploaded (gguf blocks: n/32 blocks, K-quants: n/256 super-blocks)."""
    g = block_geometry(dtype)
    return n // g[0] * g[1] if g else n * DTYPE_SIZE[dtype]
# enum xh_option
OPT_FUSE_ATTN_WO = 1
OPT_PREFILL = 2
OPT_PREFILL_GLU_SPLIT = 3
OPT_PREFILL_ATTN = 5
OPT_PREFILL_ATTN_SPLIT = 6
OPT_PREFILL_RING = 7
OPT_PREFILL_ATTN_KV8 = 8
OPT_PREFILL_RING_KV8 = 9

# enum xh_tensor_kind
EMBED, ATTN_NORM, FFN_NORM, WQ, WK, WV, WO, W1, W2, W3, FINAL_NORM, WCLS = range(12)
HYDRATE_KV_CACHE, OUTPUT_LOGITS = 0, 1
# enum xh_read (xh_debug_read)
READ_X, READ_Q, READ_HB = 0, 1, 2
# xh_gemv_shape: the matvec roles, enum xh_gemv_shape_id by id, and the over-64-KiB-LDS flag
ROLE_QKV, ROLE_GLU, ROLE_RESID, ROLE_LOGITS, ROLE_STORE = range(5)
SHAPE_NAMES = ("Q384", "PF2PB", "PF2P", "GQ", "GQL", "PF2", "W2K", "PF8", "Short", "Long")
SHAPE_BIG_LDS = 16
ACT_GELU, ACT_SILU = 0, 1


class XhConfig(ctypes.Structure):
    """POD mirror of `Config` (src/model.h:25-91)."""
    _fields_ = [("dim", ctypes.c_int32), ("hidden_dim", ctypes.c_int32), ("head_dim", ctypes.c_int32),
                ("n_layers", ctypes.c_int32), ("n_heads", ctypes.c_int32), ("n_kv_heads", ctypes.c_int32),
                ("vocab_size", ctypes.c_int32), ("max_seq_len", ctypes.c_int32), ("rope_theta", ctypes.c_float),
                ("rotary_dim", ctypes.c_int32), ("norm_eps", ctypes.c_float), ("act", ctypes.c_int32),
                ("qkv_clip", ctypes.c_float), ("tie_word_embeddings", ctypes.c_int32)]


class XhSampling(ctypes.Structure):
    """xh_sampling (include/xalm_hip.h): temperature >= 0 (0 = greedy), top_k >= 0 (0 = off),
    top_p in (0, 1] (1 = off), seed."""
    _fields_ = [("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float),
                ("seed", ctypes.c_uint64)]


class XhAttnPlan(ctypes.Structure):
    """xh_attn_plan_t (include/xalm_hip.h): the path the single-token attention takes at one kv_len."""
    _fields_ = [(n, ctypes.c_int) for n in ("fused", "nsplit", "T", "n_active", "step", "rounds_full", "rounds_last",
                                            "wph", "merge_mb", "merge_nc", "stage")]


CTL_MAX_WINDOW, CTL_MAX_BIAS = 1024, 256


class XhLogitCtl(ctypes.Structure):
    """xh_logit_ctl (include/xalm_hip.h): repeat / presence / frequency penalties over the last
    last_n tokens, min_p, and n_bias (token, value) logit biases."""
    _fields_ = [("repeat_penalty", ctypes.c_float), ("presence_penalty", ctypes.c_float),
                ("frequency_penalty", ctypes.c_float), ("last_n", ctypes.c_int32), ("min_p", ctypes.c_float),
                ("n_bias", ctypes.c_int32), ("bias_token", ctypes.c_void_p), ("bias_value", ctypes.c_void_p)]


def logit_ctl(repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, last_n=0, min_p=0.0, logit_bias=None):
    """(XhLogitCtl, the arrays it points to: keep them alive for the call).  logit_bias: a dict or
    a sequence of (token, value) pairs."""
    pairs = list(logit_bias.items()) if isinstance(logit_bias, dict) else list(logit_bias or ())
    btok = np.ascontiguousarray([int(t) for t, _ in pairs], dtype=np.int32)
    bval = np.ascontiguousarray([float(v) for _, v in pairs], dtype=np.float32)
    c = XhLogitCtl(repeat_penalty, presence_penalty, frequency_penalty, last_n, min_p, len(pairs),
                   btok.ctypes.data if pairs else None, bval.ctypes.data if pairs else None)
    return c, (btok, bval)


class XhTruncCtl(ctypes.Structure):
    """xh_trunc_ctl (include/xalm_hip.h): typical_p (1 = off), top_n_sigma (0 = off), Mirostat v2's
    tau (0 = off) and eta."""
    _fields_ = [("typical_p", ctypes.c_float), ("top_n_sigma", ctypes.c_float), ("mirostat_tau", ctypes.c_float),
                ("mirostat_eta", ctypes.c_float)]


SEQ_MAX_MATCH, SEQ_MAX_BREAKERS = 64, 1024


class XhSeqCtl(ctypes.Structure):
    """xh_seq_ctl (include/xalm_hip.h): DRY (multiplier 0 = off, base, allowed length), the n-gram ban
    (0 = off), the sequence window, the breaker ids, XTC (probability 0 = off, threshold)."""
    _fields_ = [("dry_multiplier", ctypes.c_float), ("dry_base", ctypes.c_float), ("dry_allowed_length", ctypes.c_int32),
                ("no_repeat_ngram", ctypes.c_int32), ("seq_last_n", ctypes.c_int32), ("n_breakers", ctypes.c_int32),
                ("breaker_token", ctypes.c_void_p), ("xtc_probability", ctypes.c_float), ("xtc_threshold", ctypes.c_float)]


def seq_ctl(dry_multiplier=0.0, dry_base=1.75, dry_allowed_length=2, no_repeat_ngram=0, seq_last_n=0, breakers=(),
            xtc_probability=0.0, xtc_threshold=0.1):
    """(XhSeqCtl, the array it points to: keep it alive for the call)."""
    brk = np.ascontiguousarray([int(t) for t in breakers], dtype=np.int32)
    q = XhSeqCtl(dry_multiplier, dry_base, dry_allowed_length, no_repeat_ngram, seq_last_n, int(brk.size),
                 brk.ctypes.data if brk.size else None, xtc_probability, xtc_threshold)
    return q, brk


SEQ_KEYS = ("dry_multiplier", "dry_base", "dry_allowed_length", "no_repeat_ngram", "seq_last_n", "breakers",
            "xtc_probability", "xtc_threshold")

DFA_DEAD, DFA_MAX_STATES = 0xFFFF, 65535


class XhByteDfa(ctypes.Structure):
    """xh_byte_dfa (include/xalm_hip.h): next [n_states][256] uint16 (DFA_DEAD = no transition),
    accept [n_states] uint8."""
    _fields_ = [("n_states", ctypes.c_int32), ("start", ctypes.c_int32), ("next", ctypes.c_void_p),
                ("accept", ctypes.c_void_p)]


class ByteDfa:
    """A byte DFA held as numpy arrays: next uint16 [n_states, 256], accept uint8 [n_states], start."""

    def __init__(self, next, accept, start=0):
        self.next = np.ascontiguousarray(next, dtype=np.uint16).reshape(-1, 256)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        self.start = int(start)

    @property
    def n_states(self):
        return int(self.accept.size)

    def abi(self, n_states=None):
        return XhByteDfa(self.n_states if n_states is None else n_states, self.start, self.next.ctypes.data,
                         self.accept.ctypes.data)


def pieces_blob(pieces):
    """(bytes uint8 [total], offsets uint32 [V + 1]) of a list of byte strings: the piece table of
    xh_constraint_set_vocab."""
    offsets = np.zeros(len(pieces) + 1, dtype=np.uint32)
    np.cumsum([len(p) for p in pieces], out=offsets[1:])
    blob = np.frombuffer(b"".join(pieces) or b"\0", dtype=np.uint8).copy()
    return blob, offsets


def token_pieces(tokens):
    """The pieces of a .xalm vocabulary (XalmFile.tokens()), as the host Tokenizer::pieces: the
    vocab string, and the single byte for the byte-fallback tokens, the 256 ids from <0x00> on (a
    vocabulary whose run <0x00> .. <0xFF> is not whole keeps the names)."""
    out = list(tokens)
    if b"<0x00>" in out:
        b0 = out.index(b"<0x00>")
        if out[b0:b0 + 256] == [b"<0x%02X>" % i for i in range(256)]:
            out[b0:b0 + 256] = [bytes([i]) for i in range(256)]
    return out


class XhError(RuntimeError):
    pass


_lib = None

_P = ctypes.c_void_p
_I = ctypes.c_int
_SZ = ctypes.c_size_t
_FP = ctypes.POINTER(ctypes.c_float)

_SIGNATURES = {
    "xh_create": (_I, [ctypes.POINTER(XhConfig), _I, ctypes.POINTER(_P)]),
    "xh_create_kv": (_I, [ctypes.POINTER(XhConfig), _I, _I, ctypes.POINTER(_P)]),
    "xh_kv_dtype": (_I, [_P]),
    "xh_destroy": (None, [_P]),
    "xh_last_error": (ctypes.c_char_p, [_P]),
    "xh_upload": (_I, [_P, _I, _I, _I, _P, _SZ]),
    "xh_upload_file": (_I, [_P, _I, _I, _I, ctypes.c_char_p, ctypes.c_uint64, _SZ]),
    "xh_upload_synthetic": (_I, [_P, _I, _I, _I, ctypes.c_uint64, ctypes.c_float, ctypes.c_float]),
    "xh_quantize_blocks": (_I, [_I, _P, _SZ, _P]),
    "xh_dequantize_blocks": (_I, [_I, _P, _SZ, _P]),
    "xh_kv_fill_synthetic": (_I, [_P, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_float]),
    "xh_forward": (_I, [_P, _I, _I, _I, _P]),
    "xh_decode_greedy": (_I, [_P, _I, _I, _I, _I, _P, ctypes.POINTER(_I)]),
    "xh_decode_sample": (_I, [_P, _I, _I, ctypes.POINTER(XhSampling), _I, _I, _P, ctypes.POINTER(_I)]),
    "xh_decode_sample_ext": (_I, [_P, _I, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), _P, _I, _I, _I, _P,
                                  _P, ctypes.POINTER(_I)]),
    "xh_op_sample_ext": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), _P, _I, ctypes.c_uint64,
                              _I, _P, _P, _P, _P]),
    "xh_constraint_set_vocab": (_I, [_P, _P, _P]),
    "xh_constraint_set": (_I, [_P, ctypes.POINTER(XhByteDfa)]),
    "xh_decode_sample_dfa": (_I, [_P, _I, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), _P, _I,
                                  ctypes.c_uint32, _I, _I, _P, _P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_I)]),
    "xh_op_sample_dfa": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), _P, _I,
                              ctypes.POINTER(XhByteDfa), _P, _P, ctypes.c_uint32, _I, _I, ctypes.c_uint64, _I, _P, _P, _P,
                              _P, _P]),
    "xh_decode_sample_adapt": (_I, [_P, _I, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl),
                                    ctypes.POINTER(XhTruncCtl), _P, _I, _I, ctypes.c_uint32, ctypes.c_float, _I, _I, _P, _P,
                                    ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_I)]),
    "xh_op_sample_adapt": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), ctypes.POINTER(XhTruncCtl),
                                _P, _I, ctypes.POINTER(XhByteDfa), _P, _P, ctypes.c_uint32, ctypes.c_float, _I, _I,
                                ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _FP]),
    "xh_decode_sample_seq": (_I, [_P, _I, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl),
                                  ctypes.POINTER(XhTruncCtl), ctypes.POINTER(XhSeqCtl), _P, _I, _I, ctypes.c_uint32,
                                  ctypes.c_float, _I, _I, _P, _P, ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_I)]),
    "xh_op_sample_seq": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.POINTER(XhLogitCtl), ctypes.POINTER(XhTruncCtl),
                              ctypes.POINTER(XhSeqCtl), _P, _I, ctypes.POINTER(XhByteDfa), _P, _P, ctypes.c_uint32,
                              ctypes.c_float, _I, _I, ctypes.c_uint64, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "xh_seq_adjust_host": (_I, [_P, _I, ctypes.POINTER(XhSeqCtl), _P, _I, _P, _P, _P]),
    "xh_xtc_host": (_I, [_P, _I, ctypes.c_float, ctypes.POINTER(XhSeqCtl), ctypes.c_uint64, ctypes.c_uint64, _P,
                         ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "xh_truncate_host": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.c_float, ctypes.POINTER(XhTruncCtl),
                              ctypes.c_float, _I, _P, ctypes.POINTER(_I), _FP, _FP]),
    "xh_constraint_mask": (_I, [ctypes.POINTER(XhByteDfa), _P, _P, _I, ctypes.c_uint32, _I, _I, _P, _P]),
    "xh_regex_compile": (_I, [ctypes.c_char_p, _P, _P, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "xh_adjust_logits": (_I, [_P, _I, ctypes.POINTER(XhLogitCtl), _P, _I, _P]),
    "xh_op_sample": (_I, [_P, _I, ctypes.POINTER(XhSampling), ctypes.c_uint64, _I, _P, _P]),
    "xh_philox4x32": (_I, [ctypes.c_uint64, ctypes.c_uint64, _P]),
    "xh_top_logprobs_host": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "xh_op_top_logprobs": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "xh_set_top_logprobs": (_I, [_P, _I]),
    "xh_get_top_logprobs": (_I, [_P, _I, _P, _P, _P]),
    "xh_score": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "xh_prefill": (_I, [_P, _P, _I, _I, _I, _P]),
    "xh_prefill_route": (_I, [_P, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "xh_perplexity": (_I, [_P, _P, _I, _I, _P]),
    "xh_debug_trace": (_I, [_P, _I, _P, _I, ctypes.POINTER(_I)]),
    "xh_debug_read": (_I, [_P, _I, _P, _SZ]),
    "xh_gemv_shape": (_I, [_I, _I, _I]),
    "xh_attn_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, ctypes.POINTER(XhAttnPlan)]),
    "xh_get_logits": (_I, [_P, _P]),
    "xh_reset": (_I, [_P]),
    "xh_kv_write": (_I, [_P, _I, _I, _I, _I, _P]),
    "xh_kv_read": (_I, [_P, _I, _I, _I, _I, _P]),
    "xh_kv_write8": (_I, [_P, _I, _I, _I, _I, _P]),
    "xh_kv_read8": (_I, [_P, _I, _I, _I, _I, _P]),
    "xh_kv_sink_read": (_I, [_P, _I, _P]),
    "xh_f8_e4m3_from_f32": (_I, [_P, _SZ, _P]),
    "xh_op_kv_quantize": (_I, [_P, _SZ, _P]),
    "xh_op_mha8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "xh_active_bytes": (_SZ, [_P, _SZ]),
    "xh_set_graphs": (_I, [_P, _I]),
    "xh_set_option": (_I, [_P, _I, _I]),
    "xh_get_option": (_I, [_P, _I, ctypes.POINTER(_I)]),
    "xh_op_matmul": (_I, [_P, _P, _P, _I, _I, _I]),
    "xh_op_rmsnorm": (_I, [_P, _P, _P, _I, _I, ctypes.c_float]),
    "xh_op_rope": (_I, [_P, _I, _I, _I, ctypes.c_float, _I]),
    "xh_op_mha": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "xh_op_prompt_gemm": (_I, [_P, _P, _P, _P, _I, _I, _I, _I]),
    "xh_op_prompt_attn": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "xh_op_prompt_attn8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "xh_op_prompt_attn_ring": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "xh_op_prompt_attn_ring8": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "xh_op_prompt_matmul": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, ctypes.POINTER(_I)]),
    "xh_op_prompt_weight_image": (_I, [_I, _P, _I, _I, _P, _P, _I]),
    "xh_op_prompt_stage": (_I, [_I, _P, _I, _P, _P, _I, _I, _P, _I, ctypes.c_float, _I, _I, _SZ, _P, _P, _P, _P,
                                ctypes.POINTER(_I)]),
    "xh_prompt_gemm_tile": (_I, [_I]),
    "xh_time_kernel": (_I, [_P, _I, _I, _FP]),
    "xh_kernel_bytes": (_SZ, [_P, _I, _I]),
}


def lib():
    """Load libxalm_hip.so (once).  Raises if it is absent: the product has no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise XhError(f"{HIP_LIB_PATH} not built (run `make` or __graft_entry__.build())")
        L = ctypes.CDLL(HIP_LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, ctx=None):
    if rc != 0:
        msg = lib().xh_last_error(ctx)
        raise XhError(f"xh error {rc}: {msg.decode() if msg else ''}")


def ptr(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------------------
# op-level entry points (exposed-for-tests ops, src/model.h:286-316), numpy in / out
# ------------------------------------------------------------------------------------------
def op_matmul(x: np.ndarray, w: np.ndarray, dtype: int, n: int, d: int) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w)
    out = np.empty(d, dtype=np.float32)
    check(lib().xh_op_matmul(ptr(out), ptr(x), ptr(w), dtype, n, d))
    return out


def gemv_shape(role: int, dtype: int, n: int) -> int:
    """The launch shape the decode matvec of `role` takes at input length n (xh_gemv_shape): an
    index into SHAPE_NAMES, plus SHAPE_BIG_LDS above 64 KiB of LDS; -1 = none.  No device needed."""
    return int(lib().xh_gemv_shape(role, dtype, n))


def attn_plan(head_dim: int, n_heads: int, n_kv_heads: int, max_seq_len: int, kv_dtype: int, fused: int,
              kv_len: int) -> XhAttnPlan:
    """The path the single-token attention takes at kv_len (xh_attn_plan): the split launch
    (fused = 0) or the attention side of the fused attention + Wo launch (fused = 1; raises where
    the shape has none).  No device needed."""
    p = XhAttnPlan()
    check(lib().xh_attn_plan(head_dim, n_heads, n_kv_heads, max_seq_len, kv_dtype, fused, kv_len, ctypes.byref(p)))
    return p


def quantize_blocks(dtype: int, values: np.ndarray) -> np.ndarray:
    """The converter's block quantizer (quants.py `quantize`) on the host: float32 [..., n] with
    n % 32 == 0 -> uint8 [..., n / 32 * block bytes] in the file layout (Q4_K / Q6_K: n % 256 == 0,
    the project's own quantizer, xalm_hip.h).  No device needed."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    g = block_geometry(dtype)
    if g is None or v.shape[-1] % g[0]:
        raise ValueError("quantize_blocks: a block dtype and whole blocks (32 elements, K-quants 256)")
    out = np.empty(v.shape[:-1] + (v.shape[-1] // g[0] * g[1],), dtype=np.uint8)
    check(lib().xh_quantize_blocks(dtype, ptr(v), v.size // g[0], ptr(out)))
    return out


def dequantize_blocks(dtype: int, blocks: np.ndarray) -> np.ndarray:
    """The inverse on the host (xh_dequantize_blocks): uint8 [..., k * block bytes] in the file
    layout -> float32 [..., 32 k], the values the kernels decode.  No device needed."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    g = block_geometry(dtype)
    if g is None or b.shape[-1] % g[1]:
        raise ValueError("dequantize_blocks: a block dtype and whole blocks")
    out = np.empty(b.shape[:-1] + (b.shape[-1] // g[1] * g[0],), dtype=np.float32)
    check(lib().xh_dequantize_blocks(dtype, ptr(b), b.size // g[1], ptr(out)))
    return out


def op_sample(logits: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos0: int,
              n_draws: int):
    """The device sampler on a logits vector (xh_op_sample): draws at counters pos0 .. pos0 +
    n_draws - 1; returns (tokens, n_kept), int32 [n_draws] each."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, seed)
    toks = np.empty(max(n_draws, 1), dtype=np.int32)
    kept = np.empty(max(n_draws, 1), dtype=np.int32)
    check(lib().xh_op_sample(ptr(lg), lg.size, ctypes.byref(s), pos0, n_draws, ptr(toks), ptr(kept)))
    return toks[:n_draws], kept[:n_draws]


def op_sample_ext(logits: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos0: int,
                  n_draws: int, window=(), **controls):
    """The extended draw on a logits vector (xh_op_sample_ext; controls as `logit_ctl`): draws at
    counters pos0 .. pos0 + n_draws - 1 over the fixed `window`; returns (tokens, n_kept, adjusted
    logits l' [V], log-probabilities [n_draws])."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, seed)
    c, keep = logit_ctl(**controls)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    toks = np.empty(max(n_draws, 1), dtype=np.int32)
    kept = np.empty(max(n_draws, 1), dtype=np.int32)
    adj = np.empty(lg.size, dtype=np.float32)
    lp = np.empty(max(n_draws, 1), dtype=np.float32)
    check(lib().xh_op_sample_ext(ptr(lg), lg.size, ctypes.byref(s), ctypes.byref(c), ptr(win) if win.size else None,
                                 win.size, pos0, n_draws, ptr(toks), ptr(kept), ptr(adj), ptr(lp)))
    del keep
    return toks[:n_draws], kept[:n_draws], adj, lp[:n_draws]


def adjust_logits(logits: np.ndarray, window=(), **controls) -> np.ndarray:
    """l' of xh_logit_ctl on the host (xh_adjust_logits; controls as `logit_ctl`).  No device needed."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    c, keep = logit_ctl(**controls)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    out = np.empty(lg.size, dtype=np.float32)
    check(lib().xh_adjust_logits(ptr(lg), lg.size, ctypes.byref(c), ptr(win) if win.size else None, win.size, ptr(out)))
    del keep
    return out


def regex_compile(pattern) -> ByteDfa:
    """xh_regex_compile: the trimmed byte DFA of a full-match regular expression (str: its UTF-8
    bytes).  No device needed."""
    pat = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    n, start = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().xh_regex_compile(pat, None, None, 0, ctypes.byref(n), ctypes.byref(start))
    if rc != 4:  # XH_E_NOMEM carries the size
        raise XhError(f"xh error {rc}: cannot compile {pat!r}")
    nxt = np.empty((n.value, 256), dtype=np.uint16)
    acc = np.empty(n.value, dtype=np.uint8)
    check(lib().xh_regex_compile(pat, ptr(nxt), ptr(acc), n.value, ctypes.byref(n), ctypes.byref(start)))
    return ByteDfa(nxt, acc, start.value)


def constraint_mask(dfa: ByteDfa, blob: np.ndarray, offsets: np.ndarray, state: int, stop=(-1, -1)):
    """xh_constraint_mask: (allowed uint8 [V], successor states uint16 [V]) in `state`.  No device
    needed."""
    V = offsets.size - 1
    allowed = np.empty(V, dtype=np.uint8)
    nxt = np.empty(V, dtype=np.uint16)
    d = dfa.abi()
    check(lib().xh_constraint_mask(ctypes.byref(d), ptr(blob), ptr(offsets), V, int(state), int(stop[0]), int(stop[1]),
                                   ptr(allowed), ptr(nxt)))
    return allowed, nxt


def op_sample_dfa(logits: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos0: int, n_draws: int,
                  dfa: ByteDfa, blob: np.ndarray, offsets: np.ndarray, state: int, stop=(-1, -1), window=(), **controls):
    """The constrained draw on a logits vector (xh_op_sample_dfa; controls as `logit_ctl`): every
    draw from `state`; returns (tokens, n_kept, masked logits l'' [V], successor states [n_draws],
    log-probabilities [n_draws])."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, seed)
    c, keep = logit_ctl(**controls)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    toks = np.empty(max(n_draws, 1), dtype=np.int32)
    kept = np.empty(max(n_draws, 1), dtype=np.int32)
    masked = np.empty(lg.size, dtype=np.float32)
    states = np.empty(max(n_draws, 1), dtype=np.uint32)
    lp = np.empty(max(n_draws, 1), dtype=np.float32)
    d = dfa.abi()
    check(lib().xh_op_sample_dfa(ptr(lg), lg.size, ctypes.byref(s), ctypes.byref(c), ptr(win) if win.size else None,
                                 win.size, ctypes.byref(d), ptr(blob), ptr(offsets), int(state), int(stop[0]),
                                 int(stop[1]), pos0, n_draws, ptr(toks), ptr(kept), ptr(masked), ptr(states), ptr(lp)))
    del keep
    return toks[:n_draws], kept[:n_draws], masked, states[:n_draws], lp[:n_draws]


def op_sample_adapt(logits: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos0: int, n_draws: int,
                    typical_p: float = 1.0, top_n_sigma: float = 0.0, mirostat_tau: float = 0.0, mirostat_eta: float = 0.1,
                    mu: float = 0.0, dfa: "ByteDfa | None" = None, blob=None, offsets=None, state: int = 0, stop=(-1, -1),
                    window=(), **controls):
    """The adaptive draw on a logits vector (xh_op_sample_adapt; xh_trunc_ctl's fields by name, controls
    as `logit_ctl`): every draw from `state` and `mu`, masked by `dfa` over the pieces (blob, offsets)
    when given.  Returns a dict: "tokens", "n_kept" int32 [n_draws], "states" uint32 [n_draws], "mu"
    float32 [n_draws], "kept" uint8 [V] (the set after the typical stage, before top-p), "thr" (the
    n-sigma threshold, -inf when off)."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, seed)
    c, keep = logit_ctl(**controls)
    t = XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    n = max(n_draws, 1)
    out = {"tokens": np.empty(n, dtype=np.int32), "n_kept": np.empty(n, dtype=np.int32),
           "states": np.empty(n, dtype=np.uint32), "mu": np.empty(n, dtype=np.float32),
           "kept": np.empty(lg.size, dtype=np.uint8)}
    thr = ctypes.c_float(0)
    d = dfa.abi() if dfa is not None else None
    check(lib().xh_op_sample_adapt(ptr(lg), lg.size, ctypes.byref(s), ctypes.byref(c), ctypes.byref(t),
                                   ptr(win) if win.size else None, win.size, ctypes.byref(d) if d is not None else None,
                                   ptr(blob) if d is not None else None, ptr(offsets) if d is not None else None,
                                   int(state), float(mu), int(stop[0]), int(stop[1]), pos0, n_draws, ptr(out["tokens"]),
                                   ptr(out["n_kept"]), ptr(out["states"]), ptr(out["mu"]), ptr(out["kept"]),
                                   ctypes.byref(thr)))
    del keep
    for k in ("tokens", "n_kept", "states", "mu"):
        out[k] = out[k][:n_draws]
    out["thr"] = float(thr.value)
    return out


def truncate_host(logits: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
                  typical_p: float = 1.0, top_n_sigma: float = 0.0, mirostat_tau: float = 0.0, mirostat_eta: float = 0.1,
                  mu: float = 0.0, token: int = -1):
    """The kept set of the adaptive draw on l'' [V] on the host (xh_truncate_host): (kept uint8 [V], the
    set after the typical stage and before top-p; its size; the n-sigma threshold; mu after `token`,
    mu itself with token < 0 or Mirostat off).  No device needed."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, 0)
    t = XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)
    kept = np.empty(lg.size, dtype=np.uint8)
    n, thr, mu_out = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_float(0)
    check(lib().xh_truncate_host(ptr(lg), lg.size, ctypes.byref(s), float(min_p), ctypes.byref(t), float(mu), int(token),
                                 ptr(kept), ctypes.byref(n), ctypes.byref(thr), ctypes.byref(mu_out)))
    return kept, int(n.value), float(thr.value), float(mu_out.value)


def op_sample_seq(logits: np.ndarray, temperature: float, top_k: int, top_p: float, seed: int, pos0: int, n_draws: int,
                  typical_p: float = 1.0, top_n_sigma: float = 0.0, mirostat_tau: float = 0.0, mirostat_eta: float = 0.1,
                  mu: float = 0.0, dfa: "ByteDfa | None" = None, blob=None, offsets=None, state: int = 0, stop=(-1, -1),
                  window=(), **controls):
    """The sequence-aware draw on a logits vector (xh_op_sample_seq): op_sample_adapt's arguments, with
    xh_seq_ctl's fields by name (SEQ_KEYS, as `seq_ctl`) among the controls.  Returns op_sample_adapt's
    dict with "kept" uint8 [n_draws, V] (each draw's set after XTC, before top-p) in place of its
    "kept" and "thr", and "adjusted" float32 [V] (l' after DRY and the ban, before the mask), "rep",
    "ng" int32 [V] (rep_c, ng_c), "fired" int32 [n_draws] (the XTC coin)."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = XhSampling(temperature, top_k, top_p, seed)
    q, keep_q = seq_ctl(**{k: controls.pop(k) for k in SEQ_KEYS if k in controls})
    c, keep = logit_ctl(**controls)
    t = XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    n = max(n_draws, 1)
    out = {"tokens": np.empty(n, dtype=np.int32), "n_kept": np.empty(n, dtype=np.int32),
           "states": np.empty(n, dtype=np.uint32), "mu": np.empty(n, dtype=np.float32),
           "kept": np.empty((n, lg.size), dtype=np.uint8), "adjusted": np.empty(lg.size, dtype=np.float32),
           "rep": np.empty(lg.size, dtype=np.int32), "ng": np.empty(lg.size, dtype=np.int32),
           "fired": np.empty(n, dtype=np.int32)}
    d = dfa.abi() if dfa is not None else None
    check(lib().xh_op_sample_seq(ptr(lg), lg.size, ctypes.byref(s), ctypes.byref(c), ctypes.byref(t), ctypes.byref(q),
                                 ptr(win) if win.size else None, win.size, ctypes.byref(d) if d is not None else None,
                                 ptr(blob) if d is not None else None, ptr(offsets) if d is not None else None,
                                 int(state), float(mu), int(stop[0]), int(stop[1]), pos0, n_draws, ptr(out["tokens"]),
                                 ptr(out["n_kept"]), ptr(out["states"]), ptr(out["mu"]), ptr(out["adjusted"]),
                                 ptr(out["rep"]), ptr(out["ng"]), ptr(out["kept"]), ptr(out["fired"])))
    del keep, keep_q
    for k in ("tokens", "n_kept", "states", "mu", "kept", "fired"):
        out[k] = out[k][:n_draws]
    return out


def seq_adjust_host(adjusted: np.ndarray, window=(), **seq):
    """DRY and the n-gram ban on l' [V] on the host (xh_seq_adjust_host; xh_seq_ctl's fields as
    `seq_ctl`): (l' after both stages float32 [V], rep_c int32 [V], ng_c int32 [V]).  No device needed."""
    lg = np.ascontiguousarray(adjusted, dtype=np.float32)
    q, keep_q = seq_ctl(**seq)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.int32))
    out = np.empty(lg.size, dtype=np.float32)
    rep = np.empty(lg.size, dtype=np.int32)
    ng = np.empty(lg.size, dtype=np.int32)
    check(lib().xh_seq_adjust_host(ptr(lg), lg.size, ctypes.byref(q), ptr(win) if win.size else None, win.size, ptr(out),
                                   ptr(rep), ptr(ng)))
    del keep_q
    return out, rep, ng


def xtc_host(logits: np.ndarray, temperature: float, kept: np.ndarray, seed: int, pos: int, **seq):
    """XTC on l'' [V] over the set `kept` (uint8 [V], the set C) for the draw at counter pos on the
    host (xh_xtc_host): (C after XTC uint8 [V], its size, whether the coin fired).  No device needed."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    q, keep_q = seq_ctl(**seq)
    k = np.ascontiguousarray(kept, dtype=np.uint8).copy()
    n, fired = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().xh_xtc_host(ptr(lg), lg.size, float(temperature), ctypes.byref(q), seed, pos, ptr(k), ctypes.byref(n),
                            ctypes.byref(fired)))
    del keep_q
    return k, int(n.value), bool(fired.value)


TOP_MAX = 32


def _top_logprobs(fn, logits, n_top, targets):
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    lg = lg.reshape(1, -1) if lg.ndim == 1 else lg
    rows, V = lg.shape
    ids = np.empty((rows, max(n_top, 1)), dtype=np.int32)
    lps = np.empty((rows, max(n_top, 1)), dtype=np.float32)
    if targets is None:
        check(fn(ptr(lg), V, rows, n_top, None, ptr(ids), ptr(lps), None, None))
        return ids[:, :n_top], lps[:, :n_top]
    tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int32).reshape(-1))
    if tg.size != rows:
        raise ValueError(f"{tg.size} targets for {rows} rows")
    tlp = np.empty(rows, dtype=np.float32)
    rank = np.empty(rows, dtype=np.int32)
    check(fn(ptr(lg), V, rows, n_top, ptr(tg), ptr(ids), ptr(lps), ptr(tlp), ptr(rank)))
    return ids[:, :n_top], lps[:, :n_top], tlp, rank


def top_logprobs_host(logits: np.ndarray, n_top: int, targets=None):
    """The top list of each row of logits [rows, V] (or [V]) on the host (xh_top_logprobs_host; the
    definition: XH_TOP_MAX in include/xalm_hip.h): (ids int32 [rows, n_top], log-probabilities
    float32 [rows, n_top]), and with `targets` [rows] also (their log-probabilities [rows], their
    0-based ranks [rows]).  No device needed."""
    return _top_logprobs(lib().xh_top_logprobs_host, logits, n_top, targets)


def op_top_logprobs(logits: np.ndarray, n_top: int, targets=None):
    """top_logprobs_host through the device row kernel (xh_op_top_logprobs), one workgroup per row."""
    return _top_logprobs(lib().xh_op_top_logprobs, logits, n_top, targets)


def philox4x32(seed: int, pos: int) -> np.ndarray:
    """Philox4x32-10 of key (seed & 0xffffffff, seed >> 32), counter (pos mod 2^32, 0, 0, 0): the
    sampler's generator on the host (xh_philox4x32)."""
    out = np.empty(4, dtype=np.uint32)
    check(lib().xh_philox4x32(seed, pos, ptr(out)))
    return out


def op_rmsnorm(x: np.ndarray, w: np.ndarray, dtype: int, eps: float) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w)
    out = np.empty_like(x)
    check(lib().xh_op_rmsnorm(ptr(out), ptr(x), ptr(w), dtype, x.size, eps))
    return out


def op_rope(vec: np.ndarray, head_dim: int, pos: int, theta: float, rotary_dim: int) -> np.ndarray:
    v = np.array(vec, dtype=np.float32, copy=True)
    check(lib().xh_op_rope(ptr(v), v.size, head_dim, pos, theta, rotary_dim))
    return v


def f8_e4m3_from_f32(values: np.ndarray) -> np.ndarray:
    """The element of the fp8 KV ring (xh_f8_e4m3_from_f32): float32 -> e4m3 codes, uint8 of the
    same shape.  The host definition; no device needed."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.shape, dtype=np.uint8)
    check(lib().xh_f8_e4m3_from_f32(ptr(v), v.size, ptr(out)))
    return out


def op_kv_quantize(values: np.ndarray) -> np.ndarray:
    """The same through the device function the K/V writers call (xh_op_kv_quantize)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.shape, dtype=np.uint8)
    check(lib().xh_op_kv_quantize(ptr(v), v.size, ptr(out)))
    return out


def op_mha8(kb: np.ndarray, vb: np.ndarray, q: np.ndarray, head_dim: int, kv_len: int, max_seq_len: int,
            n_heads: int, n_kv_heads: int) -> np.ndarray:
    """op_mha over fp8 rings: kb / vb e4m3 codes, uint8 [max_seq_len][n_kv_heads * head_dim]."""
    kb = np.ascontiguousarray(kb, dtype=np.uint8)
    vb = np.ascontiguousarray(vb, dtype=np.uint8)
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = np.empty(n_heads * head_dim, dtype=np.float32)
    check(lib().xh_op_mha8(ptr(out), ptr(kb), ptr(vb), ptr(q), head_dim, kv_len, max_seq_len, n_heads, n_kv_heads))
    return out


def op_mha(kb: np.ndarray, vb: np.ndarray, q: np.ndarray, head_dim: int, kv_len: int, max_seq_len: int,
           n_heads: int, n_kv_heads: int) -> np.ndarray:
    kb = np.ascontiguousarray(kb, dtype=np.uint16)
    vb = np.ascontiguousarray(vb, dtype=np.uint16)
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = np.empty(n_heads * head_dim, dtype=np.float32)
    check(lib().xh_op_mha(ptr(out), ptr(kb), ptr(vb), ptr(q), head_dim, kv_len, max_seq_len, n_heads, n_kv_heads))
    return out


def op_prompt_gemm(w: np.ndarray, xh: np.ndarray, xl: np.ndarray, ks: int = 0) -> np.ndarray:
    """The prompt-pass GEMM (gemm16.h): y[t][r] = sum_k w[r][k] (xh[t][k] + xl[t][k]); w, xh, xl
    f16 bit patterns (uint16) [rows][K], [n][K]; returns f32 [n][rows]."""
    w = np.ascontiguousarray(w, dtype=np.uint16)
    xh = np.ascontiguousarray(xh, dtype=np.uint16)
    xl = np.ascontiguousarray(xl, dtype=np.uint16)
    rows, K = w.shape
    n = xh.shape[0]
    assert xh.shape == (n, K) and xl.shape == (n, K)
    out = np.empty((n, rows), dtype=np.float32)
    check(lib().xh_op_prompt_gemm(ptr(out), ptr(w), ptr(xh), ptr(xl), rows, K, n, ks))
    return out


def op_prompt_attn(q: np.ndarray, k: np.ndarray, v: np.ndarray, pos0: int, head_dim: int, n_heads: int, n_kv_heads: int,
                   mode: int = 1, nsplit: int = 0) -> np.ndarray:
    """The causal attention of a prompt pass (xh_op_prompt_attn): q f32 [n][n_heads * head_dim]; k, v
    f16 bit patterns (uint16) [pos0 + n][n_kv_heads * head_dim]; row t attends over slots
    [0, pos0 + t].  mode / nsplit as in include/xalm_hip.h.  Returns f32 [n][n_heads * head_dim]."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k, dtype=np.uint16)
    v = np.ascontiguousarray(v, dtype=np.uint16)
    n = q.shape[0]
    assert q.shape == (n, n_heads * head_dim)
    assert k.shape == (pos0 + n, n_kv_heads * head_dim) and v.shape == k.shape
    out = np.empty_like(q)
    check(lib().xh_op_prompt_attn(ptr(out), ptr(q), ptr(k), ptr(v), n, pos0, head_dim, n_heads, n_kv_heads, mode, nsplit))
    return out


def op_prompt_attn8(q: np.ndarray, k: np.ndarray, v: np.ndarray, pos0: int, head_dim: int, n_heads: int, n_kv_heads: int,
                    mode: int = 1, nsplit: int = 0) -> np.ndarray:
    """op_prompt_attn over fp8 K/V (xh_op_prompt_attn8): k, v e4m3 codes (uint8)
    [pos0 + n][n_kv_heads * head_dim]; everything else as op_prompt_attn."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k, dtype=np.uint8)
    v = np.ascontiguousarray(v, dtype=np.uint8)
    n = q.shape[0]
    assert q.shape == (n, n_heads * head_dim)
    assert k.shape == (pos0 + n, n_kv_heads * head_dim) and v.shape == k.shape
    out = np.empty_like(q)
    check(lib().xh_op_prompt_attn8(ptr(out), ptr(q), ptr(k), ptr(v), n, pos0, head_dim, n_heads, n_kv_heads, mode, nsplit))
    return out


# enum xh_prompt_stage
(STAGE_SPLIT, STAGE_NORM_SPLIT, STAGE_RESID_NORM_SPLIT, STAGE_RESID_THEN_NORM_SPLIT, STAGE_GLU_SPLIT,
 STAGE_GLU_THEN_SPLIT, STAGE_STORE) = range(7)
# xh_op_prompt_matmul's route_out
ROUTE_ROWMAJOR, ROUTE_F32 = 0, -1


def prompt_gemm_tile(route: int) -> int:
    """Weight rows per wave (route -1 or E > 0) or workgroup (route 0) of the prompt GEMM.  No device needed."""
    return int(lib().xh_prompt_gemm_tile(route))


def op_prompt_matmul(x: np.ndarray, w: np.ndarray, dtype: int, rows: int, mode: int, ks: int = 0):
    """One GEMM of a prompt pass (xh_op_prompt_matmul): x f32 [n][K], w [rows] rows of `dtype` in the file
    layout.  Returns (y f32 [n][rows], route)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w)
    n, K = x.shape
    assert w.nbytes == rows * row_bytes(dtype, K)
    out = np.empty((n, rows), dtype=np.float32)
    route = ctypes.c_int(-99)
    check(lib().xh_op_prompt_matmul(ptr(out), ptr(x), ptr(w), dtype, rows, K, n, mode, ks, ctypes.byref(route)))
    return out, route.value


def op_prompt_weight_image(dtype: int, w: np.ndarray, rows: int, K: int, max_groups: int = 0):
    """The f16 image(s) of the row-major prompt GEMM (xh_op_prompt_weight_image): (hi, lo) uint16
    [rows][K], lo None for the one-image dtypes."""
    w = np.ascontiguousarray(w)
    assert w.nbytes == rows * row_bytes(dtype, K)
    hi = np.empty((rows, K), dtype=np.uint16)
    lo = np.empty((rows, K), dtype=np.uint16) if dtype in (Q8_0, Q4_0, Q5_0) else None
    check(lib().xh_op_prompt_weight_image(dtype, ptr(w), rows, K, ptr(hi), ptr(lo) if lo is not None else None, max_groups))
    return hi, lo


def op_prompt_stage(kind: int, n: int, dim: int, part=None, part_s=None, x=None, norm_w=None, norm_dtype: int = F32,
                    eps: float = 1e-5, act: int = ACT_SILU, layout: int = 0, out_stride: int = 0, y=None):
    """A producer or the epilogue of a prompt GEMM (xh_op_prompt_stage).  part f32 [ks][n][row].
    STAGE_STORE: returns y [n][out_stride or dim] (y: the rows before the store).  Else returns a dict:
    x (updated, the RESID kinds), inv_s [n], hi / lo uint16 [n][dim], pad (non-zero padding halves)."""
    f32 = lambda a: None if a is None else np.array(a, dtype=np.float32, order="C", copy=True)
    part, part_s, x = f32(part), f32(part_s), f32(x)
    ks = part.shape[0] if part is not None else 1
    nw = None if norm_w is None else np.ascontiguousarray(norm_w)
    P = lambda a: None if a is None else ptr(a)
    if kind == STAGE_STORE:
        yo = np.array(y, dtype=np.float32, order="C", copy=True)
        assert yo.shape == (n, out_stride or dim) and part.shape == (ks, n, dim)
        check(lib().xh_op_prompt_stage(kind, P(part), ks, P(part_s), None, n, dim, None, 0, eps, act, layout, out_stride,
                                       ptr(yo), None, None, None, None))
        return yo
    inv_s = np.empty(n, dtype=np.float32)
    hi = np.empty((n, dim), dtype=np.uint16)
    lo = np.empty((n, dim), dtype=np.uint16)
    pad = ctypes.c_int(-1)
    check(lib().xh_op_prompt_stage(kind, P(part), ks, P(part_s), P(x), n, dim, P(nw), norm_dtype, eps, act, layout, 0, None,
                                   ptr(inv_s), ptr(hi), ptr(lo), ctypes.byref(pad)))
    return {"x": x, "inv_s": inv_s, "hi": hi, "lo": lo, "pad": pad.value}


def op_prompt_attn_ring(q: np.ndarray, k_ring: np.ndarray, v_ring: np.ndarray, ks: np.ndarray, vs: np.ndarray,
                        sink_ver: np.ndarray, p0: int, n_heads: int, n_kv_heads: int, nsplit: int = 0):
    """The attention of a ring pass at head_dim 128 (xh_op_prompt_attn_ring): q f32 [m][n_heads * 128];
    k_ring, v_ring uint16 [max_seq_len][kv_dim]; ks, vs uint16 [m][kv_dim]; sink_ver uint16
    [m][2][kv_dim].  Returns (out f32 [m][n_heads * 128], the K ring and the V ring after the commit);
    the arguments are left as they were."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    kr = np.array(k_ring, dtype=np.uint16, order="C", copy=True)
    vr = np.array(v_ring, dtype=np.uint16, order="C", copy=True)
    ks = np.ascontiguousarray(ks, dtype=np.uint16)
    vs = np.ascontiguousarray(vs, dtype=np.uint16)
    sv = np.ascontiguousarray(sink_ver, dtype=np.uint16)
    m, kv_dim = ks.shape
    L = kr.shape[0]
    assert kv_dim == n_kv_heads * 128 and q.shape == (m, n_heads * 128)
    assert kr.shape == (L, kv_dim) and vr.shape == kr.shape and vs.shape == ks.shape and sv.shape == (m, 2, kv_dim)
    out = np.empty_like(q)
    check(lib().xh_op_prompt_attn_ring(ptr(out), ptr(kr), ptr(vr), ptr(q), ptr(ks), ptr(vs), ptr(sv), m, p0, L, n_heads,
                                       n_kv_heads, nsplit))
    return out, kr, vr


def op_prompt_attn_ring8(q: np.ndarray, k_ring: np.ndarray, v_ring: np.ndarray, ks: np.ndarray, vs: np.ndarray,
                         sink_ver: np.ndarray, p0: int, n_heads: int, n_kv_heads: int, nsplit: int = 0):
    """op_prompt_attn_ring over fp8 K/V (xh_op_prompt_attn_ring8): k_ring, v_ring, ks, vs and sink_ver e4m3
    codes (uint8) in the same shapes; everything else, and the return, as op_prompt_attn_ring."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    kr = np.array(k_ring, dtype=np.uint8, order="C", copy=True)
    vr = np.array(v_ring, dtype=np.uint8, order="C", copy=True)
    ks = np.ascontiguousarray(ks, dtype=np.uint8)
    vs = np.ascontiguousarray(vs, dtype=np.uint8)
    sv = np.ascontiguousarray(sink_ver, dtype=np.uint8)
    m, kv_dim = ks.shape
    L = kr.shape[0]
    assert kv_dim == n_kv_heads * 128 and q.shape == (m, n_heads * 128)
    assert kr.shape == (L, kv_dim) and vr.shape == kr.shape and vs.shape == ks.shape and sv.shape == (m, 2, kv_dim)
    out = np.empty_like(q)
    check(lib().xh_op_prompt_attn_ring8(ptr(out), ptr(kr), ptr(vr), ptr(q), ptr(ks), ptr(vs), ptr(sv), m, p0, L, n_heads,
                                        n_kv_heads, nsplit))
    return out, kr, vr
