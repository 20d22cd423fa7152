"""The one-layer configurations of the K-quant stage sweep (tests/test_kq_gpu.py, test_kq_cpu.py), in
the manner of tests/stage_cases.py and run by the same float64 stage reference (tests/stage_ref.py).

Every length is a multiple of 256 (whole super-blocks).  test_kq_cpu.py enumerates
xh_gemv_shape(role, dtype, n) over every multiple of 256 up to 32768 for QKV, the fp8-KV QKV writer,
GLU, LOGITS (n = dim) and RESID (n = hidden for W2; n = n_heads * head_dim <= 8192 for Wo) and
asserts that this table holds a case at the smallest and at the largest n of every reachable
(role, dtype, shape).  The 512-column row is the role sweep: every prologue and epilogue once at 512
columns.  Each case runs twice on the device: on an fp16 KV ring (every stage) and on an fp8 ring
(the QKV8 writer's q and K/V codes).
"""
import numpy as np

import stage_cases as SC
import stage_ref as SR
from xalm_amd import _lib as L

import kq_ref as R

KQ = (L.Q4_K, L.Q6_K)


def case(dim, hidden, heads=2, kv_heads=1):
    return SC.case(dim, hidden, heads=heads, kv_heads=kv_heads, head_dim=128, dtypes=KQ)


CASES = [
    case(512, 512, heads=4, kv_heads=1),  # the role sweep at 512 columns (Wo 512 wide too)
    # dim: QKV / QKV8 / GLU / LOGITS boundaries (Short .. 8192, GQ at 4096, Long from 8448, the raised
    # LDS limit from 14592)
    case(256, 256),
    case(4096, 256),
    case(8192, 256),
    case(8448, 256),
    case(14336, 256),
    case(14592, 256),
    case(32768, 256),
    # hidden: W2 boundaries (Long 256 .. 14080, GQL 2048 .. 14336, GQ 4096, +lds from 14592, GQL+lds 16384)
    case(256, 2048),
    case(256, 4096),
    case(256, 14080),
    case(256, 14336),
    case(256, 14592),
    case(256, 16384),
    case(256, 32768),
    # n_heads * 128: Wo boundaries up to 8192 (one KV head per q head)
    case(256, 256, heads=16, kv_heads=16),
    case(256, 256, heads=32, kv_heads=32),
    case(256, 256, heads=62, kv_heads=62),
    case(256, 256, heads=64, kv_heads=64),
    # an odd super-block count inside the staged shape, and a partial last GQL step for W2
    case(768, 256 * 11),
]


def all_cases():
    return [(c, dt) for c in CASES for dt in c.dtypes]


# ---- tests/stage_ref.py's per-dtype helpers, with the K-quants added (installed by the tests with
# monkeypatch for the duration of a test; every other dtype goes to the original) -----------------
_host_tensor, _zero_matrix, _decode64 = SR.host_tensor, SR.zero_matrix, SR.decode64


def host_tensor(rows, cols, dt, seed, mean, std):
    if dt in KQ:
        from oracle import oracle as O
        vals = np.asarray(O.synthetic(rows, cols, L.F32, seed, mean, std), np.float32).reshape(rows, cols)
        return L.quantize_blocks(dt, vals)
    return _host_tensor(rows, cols, dt, seed, mean, std)


def zero_matrix(dt, rows, cols):
    if dt in KQ:
        return L.quantize_blocks(dt, np.zeros((rows, cols), np.float32))
    return _zero_matrix(dt, rows, cols)


def decode64(dt, raw, cols):
    """(value, magnitude) in float64: the weight as the format defines it, and |d_eff q| + |m_eff|
    (Q6_K: |d sc (q - 32)|)"""
    if dt in KQ:
        raw = np.ascontiguousarray(raw)
        rows = raw.shape[0]
        blk = raw.reshape(-1, R.BYTES[dt])
        if dt == L.Q4_K:
            d, dmin, sc, mn, q = R.q4k_fields(blk)
            D = np.repeat(d.astype(np.float64)[:, None] * sc, 32, axis=1)
            M = np.repeat(dmin.astype(np.float64)[:, None] * mn, 32, axis=1)
            return (D * q - M).reshape(rows, cols), (np.abs(D * q) + np.abs(M)).reshape(rows, cols)
        d, sc, q = R.q6k_fields(blk)
        w = np.repeat(d.astype(np.float64)[:, None] * sc, 16, axis=1) * (q - 32)
        return w.reshape(rows, cols), np.abs(w).reshape(rows, cols)
    return _decode64(dt, raw, cols)


def install(monkeypatch):
    monkeypatch.setattr(SR, "host_tensor", host_tensor)
    monkeypatch.setattr(SR, "zero_matrix", zero_matrix)
    monkeypatch.setattr(SR, "decode64", decode64)
