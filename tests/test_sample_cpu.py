"""Seeded sampling without a GPU: the host generator, the C++ mirror (xalm_sample) against the
numpy reference on the case lists of the GPU tests, the skip cap of those lists on the reference
alone, and parameter validation before the device is touched."""
import ctypes
import os

import numpy as np
import pytest

import sample_ref as R
from conftest import ROOT
from xalm_amd import _lib as L

HOST_SO = os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so")
# draws per case of the mirror test at the large vocabularies (the mirror sorts the whole
# vocabulary per call); the case lists themselves are the GPU tests'
MIRROR_DRAWS = {300: R.N_DRAWS, 32000: 16, 128256: 8}


def host():
    lib = ctypes.CDLL(HOST_SO)
    lib.xalm_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(L.XhSampling), ctypes.c_uint64,
                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.xalm_host_last_error.restype = ctypes.c_char_p
    return lib


def mirror(lib, logits, t, k, p, seed, pos):
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    s = L.XhSampling(t, k, p, seed)
    tok, kept = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.xalm_sample(L.ptr(lg), lg.size, ctypes.byref(s), pos, ctypes.byref(tok), ctypes.byref(kept))
    assert rc == 0, lib.xalm_host_last_error()
    return tok.value, kept.value


def test_philox_matches_reference():
    rng = np.random.default_rng(3)
    seeds = [int(x) for x in rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)]
    poss = [int(x) for x in rng.integers(0, 2 ** 32, 1000, dtype=np.uint64)]
    seeds[:3] = [0, 1, 2 ** 64 - 1]
    poss[:3] = [0, 2 ** 32 - 1, 5]
    for i in range(900, 1000):  # pos >= 2^32: only its low 32 bits are used
        poss[i] += int(rng.integers(1, 2 ** 31)) << 32
    for s, p in zip(seeds, poss):
        assert L.philox4x32(s, p).tolist() == R.philox4x32(s, p), (s, p)
    assert L.philox4x32(9, (7 << 32) + 5).tolist() == L.philox4x32(9, 5).tolist()
    assert L.lib().xh_philox4x32(1, 1, None) == 1  # XH_E_INVALID


def test_philox_known_answer():
    # Random123 kat_vectors, philox4x32 10 rounds, counter 0, key 0
    want = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert R.philox4x32(0, 0) == want
    assert L.philox4x32(0, 0).tolist() == want


@pytest.mark.parametrize("V", R.VOCABS)
def test_skip_cap_on_reference(V):
    grid = R.grid(V)
    undecided = [c for c in grid if not R.grid_analysis(V, *c).decided]
    assert len(undecided) <= R.SKIP_CAP * len(grid), undecided


def test_edge_cases_reference():
    for name, (lg, t, k, p, kept) in R.edge_cases().items():
        an = R.Analysis(lg, t, k, p)
        assert an.decided, name
        if kept is not None:
            assert an.kept.tolist() == kept, name
        for d in range(8):
            assert an.accepted(R.SEED, R.POS0 + d), name
    assert R.Analysis(*R.edge_cases()["all_neg_inf"][:4]).accepted(1, 1) == {0}
    assert R.Analysis(*R.edge_cases()["greedy_all_tiny"][:4]).accepted(1, 1) == {0}


@pytest.mark.parametrize("V", R.VOCABS)
def test_mirror_matches_reference_grid(V):
    lib = host()
    lg = R.peaked_logits(V)
    n = 0
    for (t, k, p) in R.grid(V):
        an = R.grid_analysis(V, t, k, p)
        if not an.decided:
            continue
        for d in range(MIRROR_DRAWS[V]):
            tok, kept = mirror(lib, lg, t, k, p, R.SEED, R.POS0 + d)
            assert kept == an.n_kept, (t, k, p)
            assert tok in an.accepted(R.SEED, R.POS0 + d), (t, k, p, d, tok)
            n += 1
    assert n


def test_mirror_matches_reference_edges():
    lib = host()
    for name, (lg, t, k, p, _) in R.edge_cases().items():
        an = R.Analysis(lg, t, k, p)
        for d in range(16):
            tok, kept = mirror(lib, lg, t, k, p, R.SEED, R.POS0 + d)
            assert kept == an.n_kept, name
            assert tok in an.accepted(R.SEED, R.POS0 + d), (name, d, tok)


def test_flat_logits_without_top_p():
    # flat logits: accepted = index neighbours only
    lib = host()
    lg = np.zeros(300, np.float32)
    an = R.Analysis(lg, 1.0, 0, 1.0)
    seen = set()
    for d in range(64):
        acc = an.accepted(R.SEED, d)
        assert 1 <= len(acc) <= 2 and max(acc) - min(acc) <= 1
        tok, kept = mirror(lib, lg, 1.0, 0, 1.0, R.SEED, d)
        assert kept == 300 and tok in acc
        seen.add(tok)
    assert len(seen) > 32


BAD = [(-1.0, 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, -0.5), (1.0, 0, 1.5),
       (1.0, 0, float("nan"))]


@pytest.mark.parametrize("t,k,p", BAD)
def test_invalid_parameters_rejected_before_the_device(t, k, p):
    lib = L.lib()
    lg = np.zeros(64, np.float32)
    toks = np.zeros(4, np.int32)
    kept = np.zeros(4, np.int32)
    s = L.XhSampling(t, k, p, 1)
    assert lib.xh_op_sample(L.ptr(lg), 64, ctypes.byref(s), 0, 4, L.ptr(toks), L.ptr(kept)) == 1
    assert lib.xh_last_error(None)
    done = ctypes.c_int(-1)
    # no context exists without a device: the parameters are judged first all the same
    assert lib.xh_decode_sample(None, 0, 4, ctypes.byref(s), -1, -1, L.ptr(toks), ctypes.byref(done)) == 1
    assert done.value == 0
    tok, nk = ctypes.c_int(0), ctypes.c_int(0)
    h = host()
    assert h.xalm_sample(L.ptr(lg), 64, ctypes.byref(s), 0, ctypes.byref(tok), ctypes.byref(nk)) != 0
    assert h.xalm_host_last_error()


def test_null_pointers_rejected():
    lib = L.lib()
    lg = np.zeros(64, np.float32)
    toks = np.zeros(4, np.int32)
    kept = np.zeros(4, np.int32)
    s = L.XhSampling(1.0, 0, 1.0, 1)
    assert lib.xh_op_sample(L.ptr(lg), 64, None, 0, 4, L.ptr(toks), L.ptr(kept)) == 1
    assert lib.xh_op_sample(None, 64, ctypes.byref(s), 0, 4, L.ptr(toks), L.ptr(kept)) == 1
    assert lib.xh_op_sample(L.ptr(lg), 64, ctypes.byref(s), 0, 4, None, L.ptr(kept)) == 1
    assert lib.xh_op_sample(L.ptr(lg), 0, ctypes.byref(s), 0, 4, L.ptr(toks), L.ptr(kept)) == 1
    assert lib.xh_decode_sample(None, 0, 4, None, -1, -1, L.ptr(toks), None) == 1
    assert lib.xh_decode_sample(None, 0, 4, ctypes.byref(s), -1, -1, L.ptr(toks), None) == 1
