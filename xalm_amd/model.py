"""Host-side mirror of the reference `Model` / `InferenceState` API over the C ABI.

    model = Model.from_xalm(XalmFile(path), context=0, device=0)   # src/model.cpp:48-118
    state = InferenceState(model.config)                             # src/model.h:96-156
    model.forward(state, token, pos, mode=OUTPUT_LOGITS)             # src/model.h:272
    state.logits()                                                   # host float[vocab]

Every call goes to libxalm_hip.so (HIP kernels on gfx950); errors raise XhError, as the
reference loader throws.  There is no CPU path here.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .xalm_file import XalmFile


class InferenceState:
    """Host view of the device state: only `logits` crosses back."""

    def __init__(self, config: L.XhConfig):
        self._logits = np.zeros(config.vocab_size, dtype=np.float32)

    def logits(self) -> np.ndarray:
        return self._logits


class Model:
    def __init__(self, config: L.XhConfig, device: int = 0, kv_dtype: int = L.F16):
        """`kv_dtype`: the KV rings' element type, L.F16 or L.F8_E4M3 (xh_create_kv)."""
        self.config = config
        self._ctx = ctypes.c_void_p()
        L.check(L.lib().xh_create_kv(ctypes.byref(config), device, int(kv_dtype), ctypes.byref(self._ctx)))

    # -- construction ----------------------------------------------------------------
    @classmethod
    def from_xalm(cls, xf: XalmFile, context: int = 0, device: int = 0, direct: bool = True,
                  kv_dtype: int = L.F16) -> "Model":
        """`direct`: tensors stream from the file into device memory (xh_upload_file);
        otherwise each one is read on the host and copied (xh_upload)."""
        cfg = xf.config(context)
        m = cls(cfg, device, kv_dtype)
        c = cfg
        shapes = {L.EMBED: (c.vocab_size, c.dim), L.FINAL_NORM: (c.dim,), L.WCLS: (c.vocab_size, c.dim)}
        for kind, name in xf.global_tensors(bool(c.tie_word_embeddings)).items():
            m._load(xf, kind, 0, name, shapes[kind], direct)
        q_dim, kv_dim = c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim
        lshapes = {L.ATTN_NORM: (c.dim,), L.FFN_NORM: (c.dim,), L.WQ: (q_dim, c.dim), L.WK: (kv_dim, c.dim),
                   L.WV: (kv_dim, c.dim), L.WO: (c.dim, q_dim), L.W1: (c.hidden_dim, c.dim),
                   L.W2: (c.dim, c.hidden_dim), L.W3: (c.hidden_dim, c.dim)}
        for layer in range(c.n_layers):
            for kind, name in xf.layer_tensors(layer).items():
                m._load(xf, kind, layer, name, lshapes[kind], direct)
        return m

    def _load(self, xf: XalmFile, kind: int, layer: int, name: str, expected_shape, direct: bool = True):
        ti = xf.tensors[name]
        dt = xf.dtype(name)
        g = L.block_geometry(dt)
        if g and len(expected_shape) == 2 and expected_shape[1] % g[0] == 0:
            # gguf blocks (convert.py:176-187): the header holds the byte shape
            expected_shape = (expected_shape[0], expected_shape[1] // g[0] * g[1])
        if tuple(ti.shape) != tuple(expected_shape):  # src/model.cpp:65-76
            raise ValueError(f"shape mismatch for {name}: {ti.shape} vs {expected_shape} expected!")
        if direct:
            self.upload_file(kind, layer, xf.dtype(name), xf.path, ti.offset, ti.size)
        else:
            self.upload(kind, layer, xf.dtype(name), np.ascontiguousarray(xf.raw(name)))

    def upload(self, kind: int, layer: int, dtype: int, data: np.ndarray):
        data = np.ascontiguousarray(data)
        L.check(L.lib().xh_upload(self._ctx, kind, layer, dtype, L.ptr(data), data.nbytes), self._ctx)

    def upload_file(self, kind: int, layer: int, dtype: int, path: str, offset: int, nbytes: int):
        L.check(L.lib().xh_upload_file(self._ctx, kind, layer, dtype, str(path).encode(), int(offset), int(nbytes)),
                self._ctx)

    def upload_synthetic(self, kind: int, layer: int, dtype: int, seed: int, mean: float, std: float):
        L.check(L.lib().xh_upload_synthetic(self._ctx, kind, layer, dtype, seed, mean, std), self._ctx)

    def kv_fill_synthetic(self, layer: int, which: int, slot0: int, n_slots: int, seed: int, std: float):
        L.check(L.lib().xh_kv_fill_synthetic(self._ctx, layer, which, slot0, n_slots, seed, std), self._ctx)

    # -- inference -----------------------------------------------------------------------
    def forward(self, s: InferenceState, token: int, pos: int, mode: int = L.OUTPUT_LOGITS):
        out = L.ptr(s.logits()) if mode == L.OUTPUT_LOGITS else None
        L.check(L.lib().xh_forward(self._ctx, int(token), int(pos), int(mode), out), self._ctx)

    def decode_greedy(self, pos: int, n_steps: int, stop=(-1, -1)) -> list[int]:
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        done = ctypes.c_int(0)
        L.check(L.lib().xh_decode_greedy(self._ctx, int(pos), int(n_steps), int(stop[0]), int(stop[1]),
                                         L.ptr(toks), ctypes.byref(done)), self._ctx)
        return toks[: done.value].tolist()

    def decode_sample(self, pos: int, n_steps: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                      seed: int = 0, stop=(-1, -1)) -> list[int]:
        """The device decode loop with seeded temperature / top-k / top-p sampling (xh_sampling,
        include/xalm_hip.h): step i is drawn at counter pos + i."""
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        done = ctypes.c_int(0)
        s = L.XhSampling(temperature, top_k, top_p, seed)
        L.check(L.lib().xh_decode_sample(self._ctx, int(pos), int(n_steps), ctypes.byref(s), int(stop[0]),
                                         int(stop[1]), L.ptr(toks), ctypes.byref(done)), self._ctx)
        return toks[: done.value].tolist()

    def decode_sample_ext(self, pos: int, n_steps: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                          seed: int = 0, repeat_penalty: float = 1.0, presence_penalty: float = 0.0,
                          frequency_penalty: float = 0.0, last_n: int = 0, min_p: float = 0.0, logit_bias=None,
                          history=(), logprobs: bool = False, stop=(-1, -1)):
        """decode_sample with repetition penalties over the last `last_n` tokens of history +
        output, logit biases (a dict or (token, value) pairs; -inf bans), min-p, and the
        log-probability of each token (xh_logit_ctl, include/xalm_hip.h).  `history` = the tokens
        at the positions before `pos`.  Returns the tokens, or (tokens, log-probabilities) with
        `logprobs`."""
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        lps = np.zeros(max(n_steps, 1), dtype=np.float32)
        done = ctypes.c_int(0)
        s = L.XhSampling(temperature, top_k, top_p, seed)
        c, keep = L.logit_ctl(repeat_penalty, presence_penalty, frequency_penalty, last_n, min_p, logit_bias)
        hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32))
        L.check(L.lib().xh_decode_sample_ext(self._ctx, int(pos), int(n_steps), ctypes.byref(s), ctypes.byref(c),
                                             L.ptr(hist) if hist.size else None, int(hist.size), int(stop[0]),
                                             int(stop[1]), L.ptr(toks), L.ptr(lps), ctypes.byref(done)), self._ctx)
        del keep
        out = toks[: done.value].tolist()
        return (out, lps[: done.value].copy()) if logprobs else out

    def set_constraint_vocab(self, pieces) -> None:
        """The byte string of every token (xh_constraint_set_vocab): a list of vocab_size bytes
        objects, e.g. L.token_pieces(xf.tokens())."""
        blob, offsets = L.pieces_blob(list(pieces))
        if offsets.size - 1 != self.config.vocab_size:
            raise ValueError(f"{offsets.size - 1} pieces for a vocabulary of {self.config.vocab_size}")
        L.check(L.lib().xh_constraint_set_vocab(self._ctx, L.ptr(blob), L.ptr(offsets)), self._ctx)

    def set_constraint(self, dfa: "L.ByteDfa | None") -> None:
        """The byte DFA decode_sample_dfa masks with (xh_constraint_set); None clears it."""
        if dfa is None:
            L.check(L.lib().xh_constraint_set(self._ctx, None), self._ctx)
        else:
            d = dfa.abi()
            L.check(L.lib().xh_constraint_set(self._ctx, ctypes.byref(d)), self._ctx)

    def decode_sample_dfa(self, pos: int, n_steps: int, temperature: float, state: int, top_k: int = 0, top_p: float = 1.0,
                          seed: int = 0, repeat_penalty: float = 1.0, presence_penalty: float = 0.0,
                          frequency_penalty: float = 0.0, last_n: int = 0, min_p: float = 0.0, logit_bias=None,
                          history=(), stop=(-1, -1)):
        """decode_sample_ext under the byte-DFA constraint (xh_byte_dfa, include/xalm_hip.h): only
        tokens whose bytes the DFA can read from `state` are drawn; `stop` tokens are allowed where
        the DFA accepts.  `state` = the DFA's start, or the state a previous call returned.  Returns
        (tokens, log-probabilities, state after the last token)."""
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        lps = np.zeros(max(n_steps, 1), dtype=np.float32)
        done = ctypes.c_int(0)
        state_out = ctypes.c_uint32(0)
        s = L.XhSampling(temperature, top_k, top_p, seed)
        c, keep = L.logit_ctl(repeat_penalty, presence_penalty, frequency_penalty, last_n, min_p, logit_bias)
        hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32))
        L.check(L.lib().xh_decode_sample_dfa(self._ctx, int(pos), int(n_steps), ctypes.byref(s), ctypes.byref(c),
                                             L.ptr(hist) if hist.size else None, int(hist.size), int(state),
                                             int(stop[0]), int(stop[1]), L.ptr(toks), L.ptr(lps),
                                             ctypes.byref(state_out), ctypes.byref(done)), self._ctx)
        del keep
        return toks[: done.value].tolist(), lps[: done.value].copy(), int(state_out.value)

    def decode_sample_adapt(self, pos: int, n_steps: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                            seed: int = 0, typical_p: float = 1.0, top_n_sigma: float = 0.0, mirostat_tau: float = 0.0,
                            mirostat_eta: float = 0.1, mu: float | None = None, constrain: bool = False, state: int = 0,
                            repeat_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                            last_n: int = 0, min_p: float = 0.0, logit_bias=None, history=(), stop=(-1, -1)):
        """decode_sample_dfa with the adaptive truncation of xh_trunc_ctl (include/xalm_hip.h):
        top-n-sigma, locally typical sampling, or Mirostat v2, whose `mu` is carried on the device
        between steps (None = 2 * mirostat_tau, the start; else the mu a previous call returned).
        `constrain` masks with the uploaded constraint from `state`.  Returns (tokens,
        log-probabilities, state after the last token, mu after the last token)."""
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        lps = np.zeros(max(n_steps, 1), dtype=np.float32)
        done = ctypes.c_int(0)
        state_out = ctypes.c_uint32(0)
        mu_out = ctypes.c_float(0)
        s = L.XhSampling(temperature, top_k, top_p, seed)
        c, keep = L.logit_ctl(repeat_penalty, presence_penalty, frequency_penalty, last_n, min_p, logit_bias)
        t = L.XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)
        hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32))
        mu_in = 2.0 * mirostat_tau if mu is None else mu
        L.check(L.lib().xh_decode_sample_adapt(self._ctx, int(pos), int(n_steps), ctypes.byref(s), ctypes.byref(c),
                                               ctypes.byref(t), L.ptr(hist) if hist.size else None, int(hist.size),
                                               int(bool(constrain)), int(state), float(mu_in), int(stop[0]), int(stop[1]),
                                               L.ptr(toks), L.ptr(lps), ctypes.byref(state_out), ctypes.byref(mu_out),
                                               ctypes.byref(done)), self._ctx)
        del keep
        return toks[: done.value].tolist(), lps[: done.value].copy(), int(state_out.value), float(mu_out.value)

    def decode_sample_seq(self, pos: int, n_steps: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                          seed: int = 0, dry_multiplier: float = 0.0, dry_base: float = 1.75, dry_allowed_length: int = 2,
                          no_repeat_ngram: int = 0, seq_last_n: int = 0, breakers=(), xtc_probability: float = 0.0,
                          xtc_threshold: float = 0.1, typical_p: float = 1.0, top_n_sigma: float = 0.0,
                          mirostat_tau: float = 0.0, mirostat_eta: float = 0.1, mu: float | None = None,
                          constrain: bool = False, state: int = 0, repeat_penalty: float = 1.0,
                          presence_penalty: float = 0.0, frequency_penalty: float = 0.0, last_n: int = 0,
                          min_p: float = 0.0, logit_bias=None, history=(), stop=(-1, -1)):
        """decode_sample_adapt with the sequence-aware stages of xh_seq_ctl (include/xalm_hip.h): DRY
        (a penalty that grows with the length of the repeat a token would extend, measured over the
        last `seq_last_n` tokens of history + output and cut at `breakers`), the no-repeat-n-gram ban
        and XTC (with `xtc_probability`, drop every token above `xtc_threshold` but the least likely
        of them).  Returns what decode_sample_adapt returns."""
        toks = np.zeros(max(n_steps, 1), dtype=np.int32)
        lps = np.zeros(max(n_steps, 1), dtype=np.float32)
        done = ctypes.c_int(0)
        state_out = ctypes.c_uint32(0)
        mu_out = ctypes.c_float(0)
        s = L.XhSampling(temperature, top_k, top_p, seed)
        c, keep = L.logit_ctl(repeat_penalty, presence_penalty, frequency_penalty, last_n, min_p, logit_bias)
        t = L.XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)
        q, keep_q = L.seq_ctl(dry_multiplier, dry_base, dry_allowed_length, no_repeat_ngram, seq_last_n, breakers,
                              xtc_probability, xtc_threshold)
        hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32))
        mu_in = 2.0 * mirostat_tau if mu is None else mu
        L.check(L.lib().xh_decode_sample_seq(self._ctx, int(pos), int(n_steps), ctypes.byref(s), ctypes.byref(c),
                                             ctypes.byref(t), ctypes.byref(q), L.ptr(hist) if hist.size else None,
                                             int(hist.size), int(bool(constrain)), int(state), float(mu_in), int(stop[0]),
                                             int(stop[1]), L.ptr(toks), L.ptr(lps), ctypes.byref(state_out),
                                             ctypes.byref(mu_out), ctypes.byref(done)), self._ctx)
        del keep, keep_q
        return toks[: done.value].tolist(), lps[: done.value].copy(), int(state_out.value), float(mu_out.value)

    def prefill(self, tokens, pos0: int, s: InferenceState | None = None) -> None:
        """Hydrate tokens[0..n) at positions pos0.. (the prompt loop of run_completion,
        src/main.cpp:94-100); the last token's logits land in `s` when given."""
        toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32))
        out = L.ptr(s.logits()) if s is not None else None
        L.check(L.lib().xh_prefill(self._ctx, L.ptr(toks), int(toks.size), int(pos0), int(s is not None), out),
                self._ctx)

    def prefill_route(self, n: int, pos0: int) -> tuple[int, int]:
        """(tokens that `prefill` of n tokens at pos0 would run in batched passes, the number of
        passes) under the current options (xh_prefill_route); the rest take the per-token loop."""
        nb, npass = ctypes.c_int(0), ctypes.c_int(0)
        L.check(L.lib().xh_prefill_route(self._ctx, int(n), int(pos0), ctypes.byref(nb), ctypes.byref(npass)),
                self._ctx)
        return int(nb.value), int(npass.value)

    def token_probs(self, tokens, pos0: int = 0) -> np.ndarray:
        """run_perplexity's loop (src/main.cpp:243-254) on the device: forward tokens[:-1] at
        positions pos0.., element i = Sampler::sample_prob(tokens[i + 1]) after token i."""
        toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32))
        out = np.zeros(max(toks.size - 1, 1), dtype=np.float32)
        L.check(L.lib().xh_perplexity(self._ctx, L.ptr(toks), int(toks.size), int(pos0), L.ptr(out)), self._ctx)
        return out[: toks.size - 1]

    def set_top_logprobs(self, n_top: int) -> None:
        """n_top > 0: every device decode loop also records, per step, the n_top most likely tokens
        of the raw logits with their log-probabilities and the rank of the token it emitted
        (xh_set_top_logprobs); 0 = off, the default.  The tokens are the same either way."""
        L.check(L.lib().xh_set_top_logprobs(self._ctx, int(n_top)), self._ctx)
        self._n_top = int(n_top)

    def top_logprobs(self, n_steps: int):
        """(ids int32 [n_steps, n_top], log-probabilities float32 [n_steps, n_top], ranks int32
        [n_steps]) of the first n_steps steps of the last decode call (xh_get_top_logprobs)."""
        n_top = getattr(self, "_n_top", 0)
        ids = np.empty((max(n_steps, 1), max(n_top, 1)), dtype=np.int32)
        lps = np.empty((max(n_steps, 1), max(n_top, 1)), dtype=np.float32)
        rank = np.empty(max(n_steps, 1), dtype=np.int32)
        L.check(L.lib().xh_get_top_logprobs(self._ctx, int(n_steps), L.ptr(ids), L.ptr(lps), L.ptr(rank)), self._ctx)
        return ids[:n_steps, :n_top], lps[:n_steps, :n_top], rank[:n_steps]

    def score(self, tokens, pos0: int = 0, n_top: int = 0, echo_logits: bool = False):
        """Prompt scoring (xh_score): forward tokens[:-1] at positions pos0..; element i of the
        result describes tokens[i + 1] after token i.  Returns a dict: "logprobs" float32 [n - 1],
        "ranks" int32 [n - 1] (0 = the greedy choice), with n_top > 0 "top_ids" / "top_logprobs"
        [n - 1, n_top], with echo_logits "logits" float32 [n - 1, V], the raw logits of every row."""
        toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32))
        m = max(toks.size - 1, 1)
        out = {"logprobs": np.empty(m, dtype=np.float32), "ranks": np.empty(m, dtype=np.int32)}
        if n_top > 0:
            out["top_ids"] = np.empty((m, n_top), dtype=np.int32)
            out["top_logprobs"] = np.empty((m, n_top), dtype=np.float32)
        if echo_logits:
            out["logits"] = np.empty((m, self.config.vocab_size), dtype=np.float32)
        opt = lambda k: L.ptr(out[k]) if k in out else None  # noqa: E731
        L.check(L.lib().xh_score(self._ctx, L.ptr(toks), int(toks.size), int(pos0), int(n_top), L.ptr(out["logprobs"]),
                                 L.ptr(out["ranks"]), opt("top_ids"), opt("top_logprobs"), opt("logits")), self._ctx)
        return out

    def debug_trace(self, enable: int = -1) -> np.ndarray:
        """Timeline of the last traced attention + Wo launch, [workgroup][8] device-clock stamps
        (100 MHz, attn_wo.h); `enable` 2/0 switches tracing for later launches."""
        n = ctypes.c_int(0)
        L.check(L.lib().xh_debug_trace(self._ctx, -1, None, 0, ctypes.byref(n)), self._ctx)
        out = np.zeros(n.value, dtype=np.uint64)
        L.check(L.lib().xh_debug_trace(self._ctx, int(enable), L.ptr(out), n.value, ctypes.byref(n)), self._ctx)
        return out

    def debug_read(self, which: int) -> np.ndarray:
        """One activation buffer as the last step left it (xh_debug_read): L.READ_X the residual
        stream, L.READ_Q the clipped and roped q, L.READ_HB the GLU output."""
        c = self.config
        n = {L.READ_X: c.dim, L.READ_Q: c.n_heads * c.head_dim, L.READ_HB: c.hidden_dim}[which]
        out = np.empty(n, dtype=np.float32)
        L.check(L.lib().xh_debug_read(self._ctx, int(which), L.ptr(out), n), self._ctx)
        return out

    def get_logits(self, s: InferenceState):
        L.check(L.lib().xh_get_logits(self._ctx, L.ptr(s.logits())), self._ctx)

    def reset(self):
        L.check(L.lib().xh_reset(self._ctx), self._ctx)

    def set_graphs(self, enable: bool):
        L.check(L.lib().xh_set_graphs(self._ctx, int(enable)), self._ctx)

    def set_option(self, option: int, value: int):
        L.check(L.lib().xh_set_option(self._ctx, int(option), int(value)), self._ctx)

    def get_option(self, option: int) -> int:
        v = ctypes.c_int(0)
        L.check(L.lib().xh_get_option(self._ctx, int(option), ctypes.byref(v)), self._ctx)
        return int(v.value)

    def active_bytes(self, pos: int) -> int:
        return int(L.lib().xh_active_bytes(self._ctx, pos))

    def kv_write(self, layer: int, which: int, slot0: int, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.uint16)
        n = rows.shape[0]
        L.check(L.lib().xh_kv_write(self._ctx, layer, which, slot0, n, L.ptr(rows)), self._ctx)

    def kv_read(self, layer: int, which: int, slot0: int, n_slots: int) -> np.ndarray:
        kv_dim = self.config.n_kv_heads * self.config.head_dim
        out = np.empty((n_slots, kv_dim), dtype=np.uint16)
        L.check(L.lib().xh_kv_read(self._ctx, layer, which, slot0, n_slots, L.ptr(out)), self._ctx)
        return out

    @property
    def kv_dtype(self) -> int:
        return int(L.lib().xh_kv_dtype(self._ctx))

    def kv_write8(self, layer: int, which: int, slot0: int, rows: np.ndarray):
        """Rows of raw e4m3 codes into an fp8 KV ring (xh_kv_write8)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        L.check(L.lib().xh_kv_write8(self._ctx, layer, which, slot0, rows.shape[0], L.ptr(rows)), self._ctx)

    def kv_read8(self, layer: int, which: int, slot0: int, n_slots: int) -> np.ndarray:
        kv_dim = self.config.n_kv_heads * self.config.head_dim
        out = np.empty((n_slots, kv_dim), dtype=np.uint8)
        L.check(L.lib().xh_kv_read8(self._ctx, layer, which, slot0, n_slots, L.ptr(out)), self._ctx)
        return out

    def kv_sink_read(self, layer: int) -> np.ndarray:
        """The layer's fp16 master of K slots 0 and 1, uint16 [2][kv_dim] (fp8 KV contexts)."""
        kv_dim = self.config.n_kv_heads * self.config.head_dim
        out = np.empty((2, kv_dim), dtype=np.uint16)
        L.check(L.lib().xh_kv_sink_read(self._ctx, layer, L.ptr(out)), self._ctx)
        return out

    def time_kernel(self, which: int, iters: int) -> float:
        us = ctypes.c_float(0)
        L.check(L.lib().xh_time_kernel(self._ctx, which, iters, ctypes.byref(us)), self._ctx)
        return float(us.value)

    def kernel_bytes(self, which: int, kv_len: int) -> int:
        return int(L.lib().xh_kernel_bytes(self._ctx, which, kv_len))

    def close(self):
        if self._ctx:
            L.lib().xh_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
