"""The one-layer configurations of the stage sweep (tests/stage_ref.py, test_stages_cpu.py,
test_stages_gpu.py).

Each row is one model shape and the weight dtypes it runs with; a (row, dtype) pair is one case:
one decode step at pos HIST over HIST slots of synthetic K/V history, max_seq_len MSL.  A large
input length for one role is never paired with a large one for another, and row counts stay
small (a few heads, vocab <= 1031), so a case takes a few seconds.

The rows are decided by the dispatch, not by taste: test_stages_cpu.py enumerates
xh_gemv_shape(role, dtype, n) over every multiple of 32 up to 32768 and asserts that for every
reachable (role, dtype, shape) this table holds a case at the smallest and at the largest n that
select it, where n is `dim` for QKV / GLU / LOGITS, `hidden` for W2 and n_heads * head_dim for Wo
(launched on its own with XH_OPT_FUSE_ATTN_WO 0; every case runs that stage at both settings).
Deleting a row, or moving a threshold in launch.hip, fails that test; it then prints the rows
that are missing.

Out of scope: the fp8 `_EXACT` decode variants (matrices holding NaN / Inf codes) stay with
test_f8_decode_every_code (tests/test_ops_gpu.py); synthetic fp8 weights never hold such codes.
"""
from collections import namedtuple

from xalm_amd import _lib as L

MSL, HIST, TOKEN = 64, 40, 5
FLT_MAX = 3.4028234663852886e38

ALL = (L.F32, L.F16, L.BF16, L.F8_E4M3, L.F8_E5M2, L.Q8, L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1)
DT_NAME = {v: k for k, v in L.DTYPE_BY_NAME.items()}


def dt(names):
    return tuple(L.DTYPE_BY_NAME[n] for n in names.split())

Case = namedtuple("Case", "dim hidden heads kv_heads head_dim vocab dtypes act clip rotary tied norm_dt prefill")


def case(dim, hidden, heads=2, kv_heads=1, head_dim=32, vocab=64, dtypes=ALL, act=L.ACT_SILU, clip=FLT_MAX,
         rotary=None, tied=0, norm_dt=L.BF16, prefill=0):
    return Case(dim, hidden, heads, kv_heads, head_dim, vocab, tuple(dtypes), act, clip,
                head_dim if rotary is None else rotary, tied, norm_dt, prefill)


# -- the boundaries of the shape selection ------------------------------------------------------
# `dim` rows (QKV / GLU / LOGITS; hidden 64 or 160) and `hidden` rows (W2; dim 64 or 256): the
# dtypes named are those for which the length is the first or last of a shape (the enumeration in
# test_stages_cpu.py says which).  2 heads x 32 with one KV head unless the row is about Wo.
CASES = [
    case(32, 32, heads=1, kv_heads=1),   # the smallest model: dim, hidden and n_heads * head_dim all 32
    # dim: QKV / GLU / LOGITS boundaries
    case(1024, 160, dtypes=dt("F32")),
    case(1056, 160, dtypes=dt("F32")),
    case(2048, 160, dtypes=dt("F16 BF16")),
    case(2080, 160, dtypes=dt("F16 BF16")),
    case(4064, 160, dtypes=dt("F32 F16 BF16")),
    case(4096, 160, dtypes=ALL),
    case(8192, 64, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(8224, 64, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(9216, 64, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(9248, 64, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(9728, 64, dtypes=dt("F16 BF16")),
    case(9760, 64, dtypes=dt("F16 BF16")),
    case(9984, 64, dtypes=dt("F32")),
    case(10016, 64, dtypes=dt("F32")),
    case(14336, 64, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(14368, 64, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(15360, 64, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(15392, 64, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(15872, 64, dtypes=dt("F16 BF16")),
    case(15904, 64, dtypes=dt("F16 BF16")),
    case(16128, 64, dtypes=dt("F32")),
    case(16160, 64, dtypes=dt("F32")),
    case(32768, 64, dtypes=ALL),
    # hidden: W2 boundaries
    case(256, 992, dtypes=dt("F32")),
    case(256, 1024, dtypes=dt("F32")),
    case(256, 2016, dtypes=dt("F16 BF16")),
    case(256, 2048, dtypes=dt("F16 BF16 Q8_0 Q4_0 Q4_1 Q5_0 Q5_1")),
    case(256, 4064, dtypes=dt("F8_E4M3 F8_E5M2 Q8")),
    case(256, 4096, dtypes=ALL),
    case(256, 4128, dtypes=dt("F32 F16 BF16 F8_E4M3 F8_E5M2 Q8")),
    case(64, 14304, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(64, 14336, dtypes=dt("Q8_0 Q4_0 Q4_1 Q5_0 Q5_1")),
    case(64, 14368, dtypes=dt("Q4_0 Q4_1 Q5_0 Q5_1")),
    case(64, 15360, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(64, 15392, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0")),
    case(64, 15872, dtypes=dt("F16 BF16")),
    case(64, 15904, dtypes=dt("F16 BF16")),
    case(64, 16128, dtypes=dt("F32")),
    case(64, 16160, dtypes=dt("F32")),
    case(64, 16384, dtypes=ALL),
    case(64, 16416, dtypes=dt("F32 F16 BF16 F8_E4M3 F8_E5M2 Q8")),
    case(64, 32768, dtypes=ALL),
    # n_heads * head_dim: Wo boundaries (heads x 32, one KV head per q head: never the fused launch)
    case(256, 160, heads=31, kv_heads=31, dtypes=dt("F32")),
    case(256, 160, heads=32, kv_heads=32, dtypes=dt("F32")),
    case(256, 160, heads=63, kv_heads=63, dtypes=dt("F16 BF16")),
    case(256, 160, heads=64, kv_heads=64, dtypes=dt("F16 BF16 Q8_0 Q4_0 Q4_1 Q5_0 Q5_1")),
    case(64, 160, heads=127, kv_heads=127, dtypes=dt("F8_E4M3 F8_E5M2 Q8")),
    case(64, 160, heads=128, kv_heads=128, dtypes=ALL),
    case(64, 160, heads=129, kv_heads=129, dtypes=dt("F32 F16 BF16 F8_E4M3 F8_E5M2 Q8")),
    case(64, 160, heads=255, kv_heads=255, dtypes=dt("Q8_0 Q4_0 Q4_1 Q5_0 Q5_1")),
    case(64, 160, heads=256, kv_heads=256, dtypes=ALL),
    # balanced grids past 2048 output rows (gemv_blocks rounds the grid up to whole multiples of
    # 256): fp8 qkv (PF2PB, 3072 rows) and the gguf W1/W3 launch (GQ, 2112 rows), with Mistral's
    # head shape, 128 x 4 q heads per KV head (the fused attention + Wo launch, Wo 2048 wide)
    case(4096, 1056, heads=16, kv_heads=4, head_dim=128, dtypes=dt("F8_E4M3 F8_E5M2 Q8 Q8_0 Q4_0 Q4_1 Q5_0 Q5_1")),
    # inside a shape, where the row loops end differently: a partial last step of PF2, the
    # rmsnorm prologue past 4096 without a register image, the staged gguf W2 (11008 = 5.375 x 2048)
    case(3072, 160, dtypes=dt("F32 F16 BF16")),
    case(5120, 64, dtypes=dt("F16 F8_E4M3 Q8_0 Q4_0")),
    case(64, 11008, dtypes=dt("Q8_0 Q4_0 Q5_1")),
]

# -- edges beyond the shape boundaries: F16 and one fp8 dtype each -------------------------------
EDGE_DT = (L.F16, L.F8_E4M3)
EDGES = [
    case(256, 160, vocab=1031, dtypes=EDGE_DT),                              # odd vocab: a one-row last group
    case(256, 160, norm_dt=L.F32, dtypes=EDGE_DT),                           # F32 norm weights
    case(256, 160, act=L.ACT_GELU, dtypes=EDGE_DT),
    case(256, 160, clip=0.5, dtypes=EDGE_DT),
    case(256, 160, heads=4, kv_heads=2, head_dim=64, rotary=32, dtypes=EDGE_DT, prefill=70),  # partial rotary; 64 x 2: no fused launch
    case(256, 160, tied=1, dtypes=EDGE_DT),
    case(512, 160, heads=4, kv_heads=1, head_dim=128, dtypes=EDGE_DT),       # 128 x 4: the fused attention + Wo launch
]


def config(c):
    cfg = L.XhConfig()
    cfg.dim, cfg.hidden_dim, cfg.head_dim, cfg.n_layers = c.dim, c.hidden, c.head_dim, 1
    cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.max_seq_len = c.heads, c.kv_heads, c.vocab, MSL
    cfg.rope_theta, cfg.rotary_dim, cfg.norm_eps, cfg.act = 10000.0, c.rotary, 1e-5, c.act
    cfg.qkv_clip, cfg.tie_word_embeddings = c.clip, c.tied
    return cfg


def case_id(c, dt):
    extra = "".join([f"-v{c.vocab}" if c.vocab != 64 else "", "-gelu" if c.act == L.ACT_GELU else "",
                     "-clip" if c.clip != FLT_MAX else "", f"-rot{c.rotary}" if c.rotary != c.head_dim else "",
                     "-tied" if c.tied else "", "-normf32" if c.norm_dt == L.F32 else ""])
    return f"d{c.dim}-h{c.hidden}-{c.heads}x{c.head_dim}kv{c.kv_heads}{extra}-{DT_NAME[dt]}"


def all_cases():
    return [(c, dt) for c in CASES + EDGES for dt in c.dtypes]
