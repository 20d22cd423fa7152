"""The gguf K-quants (XH_Q4_K / XH_Q6_K) on the host: decoders against the reference's quants.py
(through tests/golden/kq_golden.npz), the C quantizer against the numpy one and against the error
bound include/xalm_hip.h states for it, rejections, files and the requant tool.  No GPU."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

import kq_ref as R
import kq_stage_cases as KC
from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.xalm_file import XalmFile

sys.path.insert(0, os.path.join(ROOT, "tools"))
import xalm_requant  # noqa: E402

DTS = {"q4_k": L.Q4_K, "q6_k": L.Q6_K}
GOLD = np.load(fixture_path("kq_golden.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_ids_and_sizes():
    assert (L.Q4_K, L.Q6_K) == (26, 27) == (R.Q4_K, R.Q6_K)
    assert L.DTYPE_BY_NAME["Q4_K"] == 26 and L.DTYPE_BY_NAME["Q6_K"] == 27
    assert L.KQ_BLOCK_BYTES == {L.Q4_K: 144, L.Q6_K: 210} == R.BYTES
    assert L.Q4_K not in L.GQ_BLOCK_BYTES and L.Q6_K not in L.GQ_BLOCK_BYTES
    assert L.row_bytes(L.Q4_K, 512) == 288 and L.row_bytes(L.Q6_K, 768) == 630


@pytest.mark.parametrize("name", sorted(DTS))
@pytest.mark.parametrize("which", ["bytes", "random"])
def test_decoders_equal_the_reference_bit_for_bit(name, which):
    dt = DTS[name]
    by, want = GOLD[f"{name}_{which}"], GOLD[f"{name}_{which}_deq"]
    assert np.isfinite(want).all()  # the forced-finite scale fields: every row counts
    assert np.array_equal(bits(R.dequantize(dt, by)), bits(want))
    assert np.array_equal(bits(L.dequantize_blocks(dt, by)), bits(want))


def test_decoder_rows_hold_every_field_value():
    _, _, sc, mn, q = R.q4k_fields(GOLD["q4_k_random"].reshape(-1, 144))
    assert set(np.unique(sc)) == set(range(64)) == set(np.unique(mn)) and set(np.unique(q)) == set(range(16))
    _, sc6, q6 = R.q6k_fields(GOLD["q6_k_random"].reshape(-1, 210))
    assert set(np.unique(sc6)) == set(range(-128, 128)) and set(np.unique(q6)) == set(range(64))


def quantizer_rows():
    rng = np.random.default_rng(77)
    rows = {"normal": rng.standard_normal((16, 768)), "constant": np.full((1, 768), -1.7),
            "positive": np.abs(rng.standard_normal((2, 768))) + 0.25, "zeros": np.zeros((1, 768))}
    out = rng.standard_normal((2, 768))
    out[0, 300] = 1e4
    out[1, 5] = -1e4
    rows["outlier"] = out
    step = rng.standard_normal((2, 768))
    step[:, 64:96] *= 2.0 ** 10
    step[1, 512:528] *= 2.0 ** -10
    rows["sub-blocks 2^10 apart"] = step
    rows["tiny"] = rng.standard_normal((1, 768)) * 2.0 ** -30
    rows["huge"] = rng.standard_normal((1, 768)) * 1e7  # d saturates at f16's largest value
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}


@pytest.mark.parametrize("name", sorted(DTS))
def test_quantizer_equals_numpy_and_keeps_its_bound(name):
    dt = DTS[name]
    assert np.array_equal(L.quantize_blocks(dt, GOLD[name + "_values"]), GOLD[name + "_bytes"])
    for what, v in quantizer_rows().items():
        by = L.quantize_blocks(dt, v)
        assert np.array_equal(by, R.quantize(dt, v)), what
        blk = by.reshape(-1, R.BYTES[dt])
        if dt == L.Q4_K:
            d, dmin, sc, mn, q = R.q4k_fields(blk)
            assert np.isfinite(d).all() and np.isfinite(dmin).all() and (d >= 0).all() and (dmin >= 0).all()
            assert sc.max() <= 63 and mn.max() <= 63 and q.max() <= 15
        else:
            d, sc, q = R.q6k_fields(blk)
            assert np.isfinite(d).all() and (d >= 0).all() and sc.min() >= 0 and q.max() <= 63
        if what == "zeros":
            assert not by.any()
        if what == "huge":
            continue  # past f16's range the scale saturates: outside the bound's premise (65504 * 63)
        err = np.abs(R.dequantize(dt, by).astype(np.float64) - v.astype(np.float64))
        bound = R.error_bound(dt, by)
        print(name, what, "max err / bound", float((err / bound).max()))
        assert np.all(err <= bound), (what, float((err / bound).max()))


def test_rejections():
    lib = L.lib()
    v = np.zeros(256, np.float32)
    out = np.zeros(210, np.uint8)
    for dt in DTS.values():
        assert lib.xh_quantize_blocks(dt, None, 1, L.ptr(out)) == 1
        assert lib.xh_quantize_blocks(dt, L.ptr(v), 1, None) == 1
        assert lib.xh_dequantize_blocks(dt, None, 1, L.ptr(v)) == 1
        assert lib.xh_dequantize_blocks(dt, L.ptr(out), 1, None) == 1
        for bad in (np.inf, -np.inf, np.nan):
            w = v.copy()
            w[200] = bad
            with pytest.raises(L.XhError):
                L.quantize_blocks(dt, w)
        with pytest.raises(ValueError):  # 288 elements: no whole super-block
            L.quantize_blocks(dt, np.zeros(288, np.float32))
        with pytest.raises(ValueError):
            L.dequantize_blocks(dt, np.zeros(R.BYTES[dt] + 18, np.uint8))
        assert L.gemv_shape(L.ROLE_STORE, dt, 4096) >= 0


@pytest.fixture(scope="module")
def requant_files(tmp_path_factory):
    td = tmp_path_factory.mktemp("kq_cpu")
    out = {}
    for t in ("q4_k", "q6_k", "q4_k_m"):
        path = str(td / f"{t}.xalm")
        xalm_requant.requant(fixture_path("small_llama_f16.xalm"), path, t)
        out[t] = path
    return out


def expected_type(recipe, name):
    if recipe == "q4_k_m":
        return "Q6_K" if name in ("embed.weight", "output.weight") or name.endswith("mlp.down.weight") else "Q4_K"
    return recipe.upper()


@pytest.mark.parametrize("recipe", ["q4_k", "q6_k", "q4_k_m"])
def test_requant_tool_and_both_readers(requant_files, recipe):
    src = XalmFile(fixture_path("small_llama_f16.xalm"))
    xf = XalmFile(requant_files[recipe])
    n_done = 0
    for name, ti in src.tensors.items():
        to = xf.tensors[name]
        if len(ti.shape) == 2 and name.endswith(".weight") and ti.type == "F16":
            want = expected_type(recipe, name)
            assert to.type.upper() == want, (name, to.type)
            dt = L.DTYPE_BY_NAME[want]
            assert tuple(to.shape) == (ti.shape[0], ti.shape[1] // 256 * R.BYTES[dt])
            w = np.ascontiguousarray(src.raw(name)).view(np.float16).astype(np.float32).reshape(ti.shape)
            assert np.array_equal(np.ascontiguousarray(xf.raw(name)).reshape(ti.shape[0], -1), R.quantize(dt, w)), name
            n_done += 1
        else:
            assert to.type == ti.type and np.array_equal(xf.raw(name), src.raw(name)), name
    assert n_done == 15
    # q / k / v and gate / up share a dtype in every layer
    for layer in range(xf.config().n_layers):
        lt = xf.layer_tensors(layer)
        assert len({xf.dtype(lt[k]) for k in (L.WQ, L.WK, L.WV)}) == 1 and xf.dtype(lt[L.W1]) == xf.dtype(lt[L.W3])
    # the C++ reader parses the types and reads the same config
    host = ctypes.CDLL(os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so"))
    host.xalm_read_config.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(L.XhConfig)]
    c = L.XhConfig()
    assert host.xalm_read_config(requant_files[recipe].encode(), 0, ctypes.byref(c)) == 0
    py = xf.config()
    assert (c.dim, c.hidden_dim, c.head_dim, c.n_layers, c.vocab_size) == (py.dim, py.hidden_dim, py.head_dim, py.n_layers, py.vocab_size)


def test_q4_k_m_model_equals_its_recorded_digest(requant_files):
    """The model file itself is too large to commit; a fresh run must give the recorded bytes."""
    with open(requant_files["q4_k_m"], "rb") as f:
        data = f.read()
    with open(fixture_path("small_llama_q4_k_m.md5")) as f:
        assert hashlib.md5(data).hexdigest() == f.read().strip()
    assert len(data) < os.path.getsize(fixture_path("small_llama_q8_0.xalm"))


def test_requant_copies_narrow_weights_through(tmp_path, capsys):
    # tiny_mistral's 64-column rows hold no super-block: every weight is copied, and the tool says so
    dst = str(tmp_path / "tm.xalm")
    assert xalm_requant.requant(fixture_path("tiny_mistral_f16.xalm"), dst, "q4_k") == 0
    assert "copied unchanged" in capsys.readouterr().out
    a, b = XalmFile(fixture_path("tiny_mistral_f16.xalm")), XalmFile(dst)
    for name in a.tensors:
        assert a.tensors[name].type == b.tensors[name].type and np.array_equal(a.raw(name), b.raw(name))


def test_stage_case_table_covers_every_reachable_shape():
    """Every (role, dtype, shape) the dispatch can select for the K-quants over whole super-blocks
    is run by tests/kq_stage_cases.py at the smallest and at the largest length that selects it."""
    table = KC.CASES
    hit = {"dim": {c.dim for c in table}, "W2": {c.hidden for c in table}, "Wo": {c.heads * c.head_dim for c in table}}
    assert all(n % 256 == 0 for key in hit for n in hit[key])
    missing, cells = [], set()
    for dt in KC.KQ:
        for role, key, nmax in ((L.ROLE_QKV, "dim", 32768), (5, "dim", 32768), (L.ROLE_GLU, "dim", 32768),
                                (L.ROLE_LOGITS, "dim", 32768), (L.ROLE_RESID, "W2", 32768), (L.ROLE_RESID, "Wo", 8192)):
            ends = {}
            for n in range(256, nmax + 1, 256):
                sh = L.gemv_shape(role, dt, n)
                assert sh >= 0, (role, dt, n)
                lo, hi = ends.get(sh, (n, n))
                ends[sh] = (min(lo, n), max(hi, n))
            for sh, (lo, hi) in ends.items():
                cells.add((role, sh))
                missing += [(dt, role, key, sh, n) for n in (lo, hi) if n not in hit[key]]
    assert not missing, missing
    names = {L.SHAPE_NAMES[sh & ~L.SHAPE_BIG_LDS] for _, sh in cells}
    assert names == {"GQ", "GQL", "Short", "Long"}, names
    assert 512 in hit["dim"] and 512 in hit["W2"] and 512 in hit["Wo"]  # the role sweep
