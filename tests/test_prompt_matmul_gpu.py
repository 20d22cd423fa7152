"""The prompt-pass GEMM routes op by op against the float64 reference of tests/prompt_gemm_ref.py, through
the launch code of the passes: xh_op_prompt_matmul (prefill_split_kernel, the weight-image kernels, gemm16.h,
prefill_gemm16_kernel, prefill_gemm_kernel, prefill_epi_kernel), xh_op_prompt_weight_image and
xh_op_prompt_stage (the split producers and the epilogue).

Every cell asserts the route it meant to hit.  Random inputs are held to test_prompt_gemm's bar,
|y - ref| <= 1e-5 sum|terms| + 1e-7; the one-hot probes and the sparse integer sums are exact by
construction (conditions checked on the CPU by tests/test_prompt_gemm_cpu.py) and compared bitwise.
With XALM_PROMPT_ERR_OUT set, the largest err / bar each route reached is written to that file
(profiles/prompt_matmul_err.txt is such a run).

Two cells of the plan cannot exist and are pinned as what the code does instead: fp8 under
XH_OPT_PREFILL 1 with K % 64 != 0 never reaches the fragment kernel (it needs K % 128 == 0, and such a K
is row-major), it takes the f32-input kernel; and XH_Q8 has no integer weights, so no exact sums.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from xalm_amd import _lib as L

import prompt_gemm_ref as R

pytestmark = pytest.mark.gpu

E_INVALID = 1
SENTINEL = np.float32(-12345.0)
NS = (1, 31, 33, 64)
MODE = {"f32": 3, "frag": 2, "rowmajor": 1}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("XALM_PROMPT_ERR_OUT")
    if not path or not WORST:
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        rev = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True,
                                      stderr=subprocess.DEVNULL).strip()
    except Exception:
        rev = "unknown"
    with open(path, "w") as f:
        f.write("# largest err / bar reached per route and stage; written by tests/test_prompt_matmul_gpu.py\n")
        f.write(f"# (XALM_PROMPT_ERR_OUT) on the tree above commit {rev}.  GEMM bar: 1e-5 sum|terms| + 1e-7;\n")
        f.write("# stage bars: x 2e-6 |x| + 1e-7, halves (2^-22 + 4e-6) |v| + 2^-38 row max.\n")
        for k in sorted(WORST):
            f.write(f"{k:28s} {WORST[k]:.6f}\n")


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def expect_route(kind, dtype):
    return -1 if kind == "f32" else 0 if kind == "rowmajor" else (8 if dtype == L.F16 else 16)


def chunk_of(kind, dtype):
    return 8 if kind == "rowmajor" else R.elems(dtype) if kind == "f32" else expect_route(kind, dtype)


CELLS = [("f32", dt) for dt in R.F32_ROUTE_DTYPES] + [("frag", dt) for dt in R.FRAG_DTYPES] + \
        [("rowmajor", dt) for dt in R.ROWMAJOR_DTYPES]
CELL_IDS = [f"{k}-{dt}" for k, dt in CELLS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kind,dtype", CELLS, ids=CELL_IDS)
def test_random_parity(kind, dtype):
    route = expect_route(kind, dtype)
    tile = L.prompt_gemm_tile(route)
    worst = 0.0
    for K, ks in R.gemm_cases(kind, dtype):
        for rows in R.row_cases(tile):
            rng = np.random.default_rng(K * 1000 + rows + dtype)
            w = R.random_weights(rng, dtype, rows, K)
            wd = R.decode_weights(dtype, w, rows, K)
            for n in NS:
                x = R.random_x(rng, n, K)
                got, r = L.op_prompt_matmul(x, w, dtype, rows, MODE[kind], ks)
                assert r == route, (K, rows, n, r)
                again, _ = L.op_prompt_matmul(x, w, dtype, rows, MODE[kind], ks)
                assert np.array_equal(bits(got), bits(again))
                xd = x.astype(np.float64)
                ref, mag = xd @ wd.T, np.abs(xd) @ np.abs(wd).T
                ratio = float((np.abs(got - ref) / (1e-5 * mag + 1e-7)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (K, rows, n, ks, ratio)
    print(f"\n{kind}-{dtype}: worst err / bar = {worst:.4f}")
    note(f"gemm {kind}", worst)


@pytest.mark.parametrize("kind,dtype", CELLS, ids=CELL_IDS)
def test_exact_probes(kind, dtype):
    """y[t][r] == W[r][k_t] bit for bit, for k_t over every chunk, slice edge and block position, with every
    code at every position and the extreme d, m and e of the block formats."""
    route = expect_route(kind, dtype)
    rows = 3 * L.prompt_gemm_tile(route) + 33
    for K, ks in R.gemm_cases(kind, dtype):
        w = R.coded_weights(dtype, rows, K, kind == "rowmajor")
        wd = R.decode_weights(dtype, w, rows, K)
        kl = R.probe_ks(K, chunk_of(kind, dtype), max(ks, 1))
        for i in range(0, len(kl), 64):
            cols = kl[i:i + 64]
            got, r = L.op_prompt_matmul(R.probe_x(cols, K), w, dtype, rows, MODE[kind], ks)
            assert r == route
            want = wd[:, cols].T.astype(np.float32) + np.float32(0.0)  # the sum starts at +0
            bad = np.argwhere(bits(got) != bits(want))
            assert bad.size == 0, (K, ks, [(cols[t], rr, got[t, rr], want[t, rr]) for t, rr in bad[:4]])


@pytest.mark.parametrize("kind,dtype", [c for c in CELLS if c[1] != L.Q8], ids=[i for i, c in zip(CELL_IDS, CELLS) if c[1] != L.Q8])
def test_exact_sparse_sums(kind, dtype):
    """Eight non-zeros per row that need both f16 halves, integer weights: the result is the integer sum in
    any order.  A lost or misplaced lo half or a mispaired A / B k fails this where the random bar passes."""
    route = expect_route(kind, dtype)
    tile = L.prompt_gemm_tile(route)
    for K, ks in R.gemm_cases(kind, dtype):
        for rows in R.row_cases(tile)[1:]:
            for n in NS:
                rng = np.random.default_rng(K + rows * 7 + n + dtype)
                x, w, v, units = R.sparse_case(rng, dtype, rows, K, n)
                got, r = L.op_prompt_matmul(x, w, dtype, rows, MODE[kind], ks)
                assert r == route
                want = (x.astype(np.float64) @ v.T.astype(np.float64)).astype(np.float32)
                bad = np.argwhere(bits(got) != bits(want))
                assert bad.size == 0, (K, ks, rows, n, [(t, rr, got[t, rr], want[t, rr]) for t, rr in bad[:4]])


def test_routes_fall_where_the_passes_send_them():
    rng = np.random.default_rng(11)
    x = R.random_x(rng, 5, 256)
    # MXFP4 with one scale outside 114 .. 140: no f16 image, the f32-input kernel under every option
    w = R.random_weights(rng, L.MXFP4, 40, 256, wide=True)
    wd = R.decode_weights(L.MXFP4, w, 40, 256)
    for mode in (1, 2, 3):
        got, r = L.op_prompt_matmul(x, w, L.MXFP4, 40, mode)
        assert r == -1
        mag = np.abs(x.astype(np.float64)) @ np.abs(wd).T
        assert np.all(np.abs(got - x.astype(np.float64) @ wd.T) <= 1e-5 * mag + 1e-7)
    # fp8 under option 1 off the 64-deep steps: K = 96 is no multiple of the fragment kernel's rings either
    for dt in (L.F8_E4M3, L.F8_E5M2):
        assert L.op_prompt_matmul(x[:, :96].copy(), R.random_weights(rng, dt, 40, 96), dt, 40, 1)[1] == -1
        assert L.op_prompt_matmul(x[:, :128].copy(), R.random_weights(rng, dt, 40, 128), dt, 40, 1)[1] == 0
        assert L.op_prompt_matmul(x[:, :128].copy(), R.random_weights(rng, dt, 40, 128), dt, 40, 2)[1] == 16
    # the affine blocks and bf16 never leave the f32-input kernel
    for dt in (L.Q4_1, L.Q5_1, L.BF16):
        for mode in (1, 2):
            assert L.op_prompt_matmul(x, R.random_weights(rng, dt, 40, 256), dt, 40, mode)[1] == -1


# ---- images ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.IMAGE_DTYPES)
@pytest.mark.parametrize("rows,K", [(40, 192), (5, 64)])
@pytest.mark.parametrize("max_groups", [0, 1])
def test_weight_images_are_exact(dtype, rows, K, max_groups):
    for w in (R.random_weights(np.random.default_rng(rows + dtype), dtype, rows, K), R.coded_weights(dtype, rows, K, True)):
        v = R.decode_weights(dtype, w, rows, K).astype(np.float32)
        hi, lo = L.op_prompt_weight_image(dtype, w, rows, K, max_groups)
        want_hi = v.astype(np.float16).view(np.uint16)
        one = lo is None
        if one:
            assert np.array_equal(want_hi.view(np.float16).astype(np.float32), v)  # one image: the value is an f16
            pairs = [("hi", hi, want_hi)]
        else:
            want_lo = (v - want_hi.view(np.float16).astype(np.float32)).astype(np.float16).view(np.uint16)
            # a zero weight of a block with d < 0 decodes to -0; the Q8_0 image holds +0 there (measured: 18 of
            # 7680 elements, all of them -0 against +0, nothing else).  A zero's sign never reaches a sum that
            # starts at +0, so the two-image formats' zeros are compared as +0; every other element bit for bit.
            z = lambda a: np.where(a == 0x8000, np.uint16(0), a)
            pairs = [("hi", z(hi), z(want_hi)), ("lo", z(lo), z(want_lo))]
            got = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
            assert np.array_equal(got, v.astype(np.float64))  # hi + lo == v exactly
        for name, g, want in pairs:
            bad = np.argwhere(g != want)
            assert bad.size == 0, (name, [(r, k, hex(g[r, k]), hex(want[r, k]), float(v[r, k])) for r, k in bad[:6]])


# ---- stages ----------------------------------------------------------------------------------------
def stage_bar(v):
    """(2^-22 + 4e-6) |v|: the header's split bound plus twice test_rmsnorm's f32 bar; the header's bound
    holds down to lo's f16 subnormal floor, 2^-38 of the row max."""
    return (2.0 ** -22 + 4e-6) * np.abs(v) + 2.0 ** -38 * np.abs(v).max(axis=1, keepdims=True)


def check_halves(key, o, v, n):
    assert o["pad"] == 0
    assert np.all(np.isfinite(o["inv_s"])) and np.all(o["inv_s"] > 0)
    got = R.halves_value(o["hi"], o["lo"], o["inv_s"])
    ratio = float((np.abs(got - v) / (stage_bar(v) + 1e-300)).max())
    note(key, ratio)
    assert ratio <= 1.0, (key, ratio)
    zero = ~np.any(v != 0, axis=1)
    assert not o["hi"][zero].any() and not o["lo"][zero].any()


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32 if a[k].dtype == np.float32 else a[k].dtype),
                              b[k].view(np.uint32 if b[k].dtype == np.float32 else b[k].dtype)) for k in ("hi", "lo", "inv_s", "x")
               if a[k] is not None)


def norm_weight(rng, dim, dtype):
    wf = (1 + 0.1 * rng.standard_normal(dim)).astype(np.float32)
    return wf if dtype == L.F32 else (wf.view(np.uint32) >> 16).astype(np.uint16)


STAGE_SHAPES = [(n, ks, ps) for n in (1, 33) for ks in (1, 3) for ps in (False, True)]


# every width with every layout that can hold it: a fragment layout holds whole chunk pairs (2 x layout
# columns), so 1032 = 8 x 129 columns exist row-major only
DIM_LAYOUTS = [(d, l) for d in (32, 96, 1032) for l in (0, 8, 16) if d % (2 * l or 8) == 0]


@pytest.mark.parametrize("dim,layout", DIM_LAYOUTS)
def test_split_and_norm_stages(dim, layout):
    for n in (1, 33):
        rng = np.random.default_rng(dim + n + layout)
        x = R.random_x(rng, n, dim)
        if n > 1:
            x[n // 2] = 0.0  # an all-zero row: finite inv_s, zero halves
        o = L.op_prompt_stage(L.STAGE_SPLIT, n, dim, x=x, layout=layout)
        hi, lo, inv_s = R.split_exact(x)
        assert o["pad"] == 0
        assert np.array_equal(o["hi"], hi) and np.array_equal(o["lo"], lo) and np.array_equal(bits(o["inv_s"]), bits(inv_s))
        for ndt in (L.F32, L.BF16):
            nw = norm_weight(rng, dim, ndt)
            o = L.op_prompt_stage(L.STAGE_NORM_SPLIT, n, dim, x=x, norm_w=nw, norm_dtype=ndt, eps=1e-5, layout=layout)
            check_halves("stage norm halves", o, R.rmsnorm64(x, nw, ndt, 1e-5), n)


@pytest.mark.parametrize("dim,layout", DIM_LAYOUTS)
def test_resid_norm_stage_fused_equals_two_launches(dim, layout):
    for n, ks, with_ps in STAGE_SHAPES:
        rng = np.random.default_rng(dim * 3 + n + ks + layout)
        x0 = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
        # partials of x's sign: the residual add does not cancel, so its f32 error stays relative
        part = (np.abs(rng.standard_normal((ks, n, dim))) / ks * np.sign(x0)).astype(np.float32)
        if n > 1:
            x0[n // 2] = 0.0
            part[:, n // 2] = 0.0
        ps = rng.uniform(0.5, 2.0, n).astype(np.float32) if with_ps else None
        ndt = L.BF16 if ks == 3 else L.F32
        nw = norm_weight(rng, dim, ndt)
        kw = dict(part=part, part_s=ps, x=x0, norm_w=nw, norm_dtype=ndt, eps=1e-5, layout=layout)
        fused = L.op_prompt_stage(L.STAGE_RESID_NORM_SPLIT, n, dim, **kw)
        two = L.op_prompt_stage(L.STAGE_RESID_THEN_NORM_SPLIT, n, dim, **kw)
        assert same_bits(fused, two), (n, ks, with_ps)
        xr = x0.astype(np.float64) + R.sum_slices64(part, ps)
        xerr = np.abs(fused["x"] - xr) / (2e-6 * np.abs(xr) + 1e-7)
        note("stage resid x", xerr.max())
        assert xerr.max() <= 1.0
        check_halves("stage resid halves", fused, R.rmsnorm64(xr, nw, ndt, 1e-5), n)


@pytest.mark.parametrize("layout", [0, 8, 16])
@pytest.mark.parametrize("hidden", [32, 1056])
@pytest.mark.parametrize("act", [L.ACT_SILU, L.ACT_GELU])
def test_glu_stage_fused_equals_two_launches(hidden, layout, act):
    for n, ks, with_ps in STAGE_SHAPES:
        rng = np.random.default_rng(hidden + n + ks + layout + act)
        # g in -1.5 .. 3: below that 1 + tanh and 1 + e^-g cancel and no f32 formula keeps 4e-6 relative
        g = rng.uniform(-1.5, 3.0, (n, hidden))
        u = rng.standard_normal((n, hidden))
        row = np.stack([g, u], axis=-1).reshape(n, 2 * hidden)  # g / u interleaved
        wts = np.array([1.0]) if ks == 1 else np.array([0.5, 0.3, 0.2])
        part = (row[None] * wts[:, None, None]).astype(np.float32)
        if n > 1:
            part[:, n // 2] = 0.0
        ps = rng.uniform(0.5, 2.0, n).astype(np.float32) if with_ps else None
        if ps is not None:
            part = (part / ps[None, :, None]).astype(np.float32)  # keeps g in its range
        kw = dict(part=part, part_s=ps, act=act, layout=layout)
        fused = L.op_prompt_stage(L.STAGE_GLU_SPLIT, n, hidden, **kw)
        two = L.op_prompt_stage(L.STAGE_GLU_THEN_SPLIT, n, hidden, **kw)
        assert same_bits(fused, two), (n, ks, with_ps)
        s = R.sum_slices64(part, ps)
        check_halves("stage glu halves", fused, R.glu64(s[:, 0::2], s[:, 1::2], act), n)


@pytest.mark.parametrize("rows,stride", [(33, 0), (33, 40), (1031, 1040)])
def test_store_epilogue_odd_rows_and_stride(rows, stride):
    for n, ks, with_ps in STAGE_SHAPES:
        rng = np.random.default_rng(rows + n + ks)
        part = rng.standard_normal((ks, n, rows)).astype(np.float32)
        ps = rng.uniform(0.5, 2.0, n).astype(np.float32) if with_ps else None
        y0 = np.full((n, stride or rows), SENTINEL, np.float32)
        y = L.op_prompt_stage(L.STAGE_STORE, n, rows, part=part, part_s=ps, out_stride=stride, y=y0)
        want = np.zeros((n, rows), np.float32)
        for s in range(ks):  # slice order, f32
            want = want + part[s]
        if ps is not None:
            want = want * ps[:, None]
        assert np.array_equal(bits(y[:, :rows]), bits(want))
        assert np.all(y[:, rows:] == SENTINEL)


# ---- rejections --------------------------------------------------------------------------------------
def last_error():
    msg = L.lib().xh_last_error(None)
    return msg.decode() if msg else ""


def matmul_rc(dtype, rows, K, n, mode, ks, w=None, null=None):
    x = np.zeros((max(n, 1), max(K, 1)), np.float32)
    w = np.zeros(max(rows, 1) * max(K, 1) * 4, np.uint8) if w is None else w
    y = np.full((max(n, 1), max(rows, 1)), SENTINEL, np.float32)
    route = ctypes.c_int(-99)
    args = [L.ptr(y), L.ptr(x), L.ptr(w)]
    if null is not None:
        args[null] = None
    rc = L.lib().xh_op_prompt_matmul(*args, dtype, rows, K, n, mode, ks, ctypes.byref(route))
    return rc, y, route.value


@pytest.mark.parametrize("dtype,rows,K,n,mode,ks", [
    (L.U8, 64, 64, 4, 1, 0),        # no prompt GEMM for the dtype
    (99, 64, 64, 4, 1, 0),
    (L.F16, 64, 72, 4, 1, 0),       # K not in whole chunk pairs (16)
    (L.Q4_0, 64, 96, 4, 3, 0),      # nibble blocks: 64
    (L.F32, 64, 12, 4, 3, 0),
    (L.BF16, 64, 64, 65, 1, 0),     # 65 tokens off the row-major route
    (L.F16, 64, 128, 65, 2, 0),
    (L.F16, 64, 128, 4, 0, 0),      # modes
    (L.F16, 64, 128, 4, 4, 0),
    (L.F16, 64, 128, 4, 1, 3),      # forced slicings the pickers never take
    (L.F16, 64, 128, 4, 1, 4),      # 4 slices of 32
    (L.F16, 64, 1024, 4, 1, 16),    # more than 8 on the row-major route
    (L.F16, 64, 64, 4, 2, 2),       # fragments: slices of whole 64-deep rings
    (L.F32, 64, 64, 4, 3, 4),       # f32 input: K % 32 == 0, so slices of whole 32-deep rings
    (L.F32, 64, 24, 4, 3, 2),       # 6E: slices of whole chunk pairs, 3 of them
    (L.F16, 64, 128, 4, 1, 65),
    (L.F16, 0, 128, 4, 1, 0),
    (L.F16, 64, 128, 0, 1, 0),
], ids=str)
def test_prompt_matmul_rejects(dtype, rows, K, n, mode, ks):
    rc, y, route = matmul_rc(dtype, rows, K, n, mode, ks)
    assert rc == E_INVALID and last_error()
    assert np.all(y == SENTINEL) and route == -99  # nothing ran


def test_prompt_matmul_rejects_nan_blocks_and_null_pointers():
    w = R.pack_blocks(L.MXFP4, np.zeros((8, 64), int), e=np.array([[127, 255]] * 8))
    for mode in (1, 2, 3):
        rc, y, route = matmul_rc(L.MXFP4, 8, 64, 4, mode, 0, w=w)
        assert rc == E_INVALID and "255" in last_error() and np.all(y == SENTINEL) and route == -99
    for null in (0, 1, 2):
        rc, y, _ = matmul_rc(L.F16, 64, 128, 4, 1, 0, null=null)
        assert rc == E_INVALID and last_error() and np.all(y == SENTINEL)
    x = np.zeros((4, 128), np.float32)
    assert L.lib().xh_op_prompt_matmul(L.ptr(x), L.ptr(x), L.ptr(x), L.F16, 4, 128, 4, 1, 0, None) == E_INVALID


def test_weight_image_and_stage_reject():
    hi = np.full((8, 64), 0xABCD, np.uint16)
    lo = hi.copy()
    w = np.zeros(8 * 64 * 4, np.uint8)
    lib = L.lib()
    assert lib.xh_op_prompt_weight_image(L.F16, L.ptr(w), 8, 64, L.ptr(hi), None, 0) == E_INVALID       # no image
    assert lib.xh_op_prompt_weight_image(L.Q4_1, L.ptr(w), 8, 64, L.ptr(hi), L.ptr(lo), 0) == E_INVALID  # affine
    assert lib.xh_op_prompt_weight_image(L.Q8_0, L.ptr(w), 8, 64, L.ptr(hi), None, 0) == E_INVALID      # two images
    assert lib.xh_op_prompt_weight_image(L.F8_E4M3, L.ptr(w), 8, 48, L.ptr(hi), None, 0) == E_INVALID
    nan = np.full(8 * 64, 0x7F, np.uint8)
    assert lib.xh_op_prompt_weight_image(L.F8_E4M3, L.ptr(nan), 8, 64, L.ptr(hi), None, 0) == E_INVALID  # NaN codes
    wide = R.pack_blocks(L.MXFP4, np.zeros((8, 64), int), e=np.array([[127, 100]] * 8))
    assert lib.xh_op_prompt_weight_image(L.MXFP4, L.ptr(wide), 8, 64, L.ptr(hi), None, 0) == E_INVALID
    assert last_error() and np.all(hi == 0xABCD) and np.all(lo == 0xABCD)
    x = np.zeros((4, 64), np.float32)
    for kind, dim, layout in ((7, 64, 0), (L.STAGE_SPLIT, 44, 0), (L.STAGE_SPLIT, 72, 8), (L.STAGE_SPLIT, 64, 4), (L.STAGE_SPLIT, 64, 32)):
        pad = ctypes.c_int(-1)
        rc = lib.xh_op_prompt_stage(kind, None, 1, None, L.ptr(x), 4, dim, None, 0, 1e-5, 0, layout, 0, None, L.ptr(x),
                                    L.ptr(hi), L.ptr(lo), ctypes.byref(pad))
        assert rc == E_INVALID and pad.value == -1
    assert np.all(hi == 0xABCD)
