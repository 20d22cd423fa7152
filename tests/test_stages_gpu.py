"""Stage-by-stage float64 parity of the fused decode matvecs at every launch shape.

Every case of tests/stage_cases.py: one decode step of a one-layer model on the device, each of
its stages (QKV, attention + Wo fused and split, GLU, W2, LOGITS, and the greedy step's argmax)
against tests/stage_ref.py at the op bar.  A failure names the stage, the dtype, the input length,
the shape id and the worst err / bar.
"""
import numpy as np
import pytest

from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model

import bars
import stage_cases as SC
import stage_ref as SR

pytestmark = pytest.mark.gpu


def build(c, wdt, W, zero_w2=False):
    gm = Model(SC.config(c))
    for kind, dt, seed, mean, std in SR.tensor_specs(c, wdt):
        if kind == L.W2 and zero_w2:
            gm.upload(kind, 0, dt, SR.zero_matrix(dt, c.dim, c.hidden))
        elif dt == L.Q8:
            gm.upload(kind, 0, dt, W[kind][1])
        else:
            gm.upload_synthetic(kind, 0, dt, seed, mean, std)
    for which in (0, 1):
        gm.kv_fill_synthetic(0, which, 0, SC.HIST, SR.KV_SEED[which], 1.0)
    return gm


def observe(c, wdt, W):
    o = SR.Obs()
    gz = build(c, wdt, W, zero_w2=True)  # x1 + 0: the residual stream after attention + Wo
    o.x1 = {}
    for fuse in (0, 1):
        gz.set_option(L.OPT_FUSE_ATTN_WO, fuse)
        gz.forward(None, SC.TOKEN, SC.HIST, L.HYDRATE_KV_CACHE)
        o.x1[fuse] = gz.debug_read(L.READ_X)
    gz.close()
    gm = build(c, wdt, W)
    st = InferenceState(gm.config)
    gm.forward(st, SC.TOKEN, SC.HIST, L.OUTPUT_LOGITS)
    o.q, o.hb, o.x2 = gm.debug_read(L.READ_Q), gm.debug_read(L.READ_HB), gm.debug_read(L.READ_X)
    o.k_row, o.v_row = (gm.kv_read(0, which, SC.HIST, 1)[0] for which in (0, 1))
    for which in (0, 1):  # the step left the history as it was
        assert np.array_equal(gm.kv_read(0, which, 0, SC.HIST), SR.history(c, which))
    o.logits = st.logits().copy()
    o.greedy = gm.decode_greedy(SC.HIST + 1, 1)[0]
    return o, gm, st


def shape_ids(c, wdt):
    q_dim = c.heads * c.head_dim
    return {"q": (L.ROLE_QKV, c.dim), "k": (L.ROLE_QKV, c.dim), "v": (L.ROLE_QKV, c.dim), "x1_fused": (L.ROLE_RESID, q_dim),
            "x1_split": (L.ROLE_RESID, q_dim), "hb": (L.ROLE_GLU, c.dim), "x2": (L.ROLE_RESID, c.hidden),
            "logits": (L.ROLE_LOGITS, c.dim)}


def check_prefill(c, wdt, W, gm, st):
    """A prompt of c.prefill tokens from pos 0 (longer than the ring: it wraps and takes the token
    loop with sinks) against the oracle's token loop, at the north-star bar."""
    om = O.OracleModel(gm.config)
    for kind, (dt, arr) in W.items():
        om.set_tensor(kind, 0, dt, arr)
        if kind == L.EMBED and c.tied:
            om.set_tensor(L.WCLS, 0, dt, arr)
    toks = [1] + [3 + (7 * i) % (c.vocab - 3) for i in range(c.prefill - 1)]
    for pos, t in enumerate(toks):
        om.forward(t, pos, L.OUTPUT_LOGITS if pos == len(toks) - 1 else L.HYDRATE_KV_CACHE)
    gm.reset()
    gm.prefill(toks, 0, st)
    ref = om.logits()
    err = float(np.abs(st.logits() - ref).max())
    print(f"prefill {len(toks)} tokens: err {err:.3g} bar {bars.north(ref):.3g}")
    assert err <= bars.north(ref), ("prefill", err, bars.north(ref))
    om.close()


@pytest.mark.parametrize("c,wdt", SC.all_cases(), ids=[SC.case_id(c, d) for c, d in SC.all_cases()])
def test_stages(c, wdt):
    W = SR.host_weights(c, wdt)
    o, gm, st = observe(c, wdt, W)
    try:
        ratio = SR.check_stages(c, wdt, W, o)
        ids = shape_ids(c, wdt)
        report = {s: (SC.DT_NAME[wdt], ids[s][1], L.gemv_shape(ids[s][0], wdt, ids[s][1]), round(r, 4))
                  for s, r in ratio.items()}
        print("stage: (dtype, n, shape id, worst err / bar)", report)
        bad = {s: v for s, v in report.items() if not ratio[s] <= 1.0}
        assert not bad, bad
        if c.prefill:
            check_prefill(c, wdt, W, gm, st)
    finally:
        gm.close()
