"""What tests/test_dp_shapes_host.py (CPU) and tests/test_gpu_dp_shapes.py (GPU) share: the cases and the batches of the four
data-parallel exchange forms (row exchange with dp_local 0 / 1, dense all-reduce, row-sharded propagation, column shards) on
the 300 x 600 graph, the hand-set rows and the storage modes of tests/storage_cases.py.  Test infrastructure, no GPU.

A case is a storage_cases tuple (mode, d, K, dense_last, hub_nnz, reg_rows) + (world, form, B): form = rows0 | rows1 (the row
exchange with lgcn_ctx_set_dp_local 0 / 1) | dense | row_sharded | cols, B = the context's capacity and the epoch's global batch
(MAX_BATCH).  d is the FULL embedding width; a column-sharded rank holds d / world of it.

BATCHES.  Five batches per case, BATCH_SIZES = (300, 65, 37, 5, 1) triplets: shards ceil(B / W) of 150 / 100 / 75, 33 / 22 / 17,
19 / 13 / 10, 3 / 2 / 2 and 1 for W = 2 / 3 / 4.  They start from storage_cases.make_batches' draws (users and items from 1, the
big and the isolated item never drawn); the batches of more than 18 triplets then get the SPECIALS below, special j at slot
(j mod W) S + j div W of the batch -- consecutive specials in consecutive ranks' shards, so the hub user (special 0), the hub item
as positive (1) and as negative (2) lie in the shards of ranks 0, 1 and 2 mod W, item 21 is a positive in every rank's shard and
a negative in one, user 33 is named by two ranks, and the zero / tiny / outlier / subnormal rows, the pos = neg pair, the isolated
item and the last user / item are spread over the ranks.  check_case() states what a case's batches must have (a ragged last
shard, an empty trailing rank for W >= 3, none at W = 2 for B >= 2, shared row ids, hub rows on different ranks, a shard that is no
multiple of 8 slots, B > 64 and B > 128); it runs at import for every case of every grid and again in the host test."""
import numpy as np

import storage_cases as SC

BATCH_SIZES = (300, 65, 37, 5, 1)
MAX_BATCH = 300
FORMS = ("rows0", "rows1", "dense", "row_sharded", "cols")
MANY_ITEM, TWICE_USER = 21, 33
# (field, id) placed at slot slot_of(j, ..): 'pn' copies the slot's positive into its negative
SPECIALS = [("u", SC.HUB_USER), ("p", SC.HUB_ITEM), ("n", SC.HUB_ITEM), ("p", MANY_ITEM), ("p", MANY_ITEM), ("p", MANY_ITEM),
            ("p", MANY_ITEM), ("u", TWICE_USER), ("u", TWICE_USER), ("pn", None), ("u", SC.ZERO_USER), ("u", SC.TINY_USER),
            ("p", SC.OUTLIER_ITEM), ("n", SC.SUBNORMAL_ITEM), ("n", SC.ISOLATED_ITEM), ("u", SC.N_USERS - 1), ("p", SC.M_ITEMS - 1),
            ("n", MANY_ITEM)]
MIN_SPECIAL_BATCH = 19


def shard_size(B, world):                     # parallel.shard_size / shard_bounds, restated (this module imports no package)
    return (B + world - 1) // world


def shard_bounds(B, world, rank):
    S = shard_size(B, world)
    lo = min(rank * S, B)
    return lo, min(lo + S, B)


def rotate_item_ranges(ranges):
    """A row-range table [world, 4] with the item ranges handed on by one rank: rank r keeps its user rows and owns the item rows
    parallel.row_ranges gave rank r - 1.  Still a tiling of [0, N), which is all lgcn_train_epoch_dp asks of its row_ranges.  The hub
    user and the hub item are BOTH row 0 of their block, which parallel.row_ranges always gives to rank 0; under this table rank 0
    owns the hub user and rank 1 the hub item, so the hub cases of the row-sharded loop run on it."""
    out = np.array(ranges, np.int64, copy=True)
    out[:, 2:] = np.roll(out[:, 2:], 1, axis=0)
    return out


def storage_case(c):
    return tuple(c[:6])


def case_id(c):
    return f"{c[7]}-w{c[6]}-" + SC.case_id(storage_case(c))


def slot_of(j, B, world):
    S = shard_size(B, world)
    return (j % world) * S + j // world


def make_batches(case):
    """The five batches of a case -> [(users, pos, neg)] int64 arrays (module docstring)."""
    d, K, world = case[1], case[2], case[6]
    rng = np.random.Generator(np.random.PCG64(7000 + 10 * d + K + 100 * world))
    out = []
    for nb in BATCH_SIZES:
        u = rng.integers(1, SC.N_USERS, nb); p = rng.integers(1, SC.M_ITEMS, nb); n = rng.integers(1, SC.M_ITEMS, nb)
        for a in (p, n):                                              # the big row propagates, no slot names it (no saturated sigmoid)
            a[(a == SC.BIG_ITEM) | (a == SC.ISOLATED_ITEM)] = 20
        if nb >= MIN_SPECIAL_BATCH:
            field = {"u": u, "p": p, "n": n}
            for j, (f, v) in enumerate(SPECIALS):
                s = slot_of(j, nb, world)
                lo, hi = shard_bounds(nb, world, j % world)
                assert lo <= s < hi, (case, nb, j, s)
                if f == "pn":
                    n[s] = p[s]
                else:
                    field[f][s] = v
        out.append((u, p, n))
    return out


def _ranks_naming(arr, value, B, world):
    return {r for r in range(world) if (arr[slice(*shard_bounds(B, world, r))] == value).any()}


def check_case(case, batches=None):
    """The conditions a case's batches are chosen for; AssertionError names the one that fails."""
    world, form, hub = case[6], case[7], case[4]
    assert form in FORMS and case[8] == MAX_BATCH
    batches = make_batches(case) if batches is None else batches
    sizes = [len(b[0]) for b in batches]
    assert tuple(sizes) == BATCH_SIZES and max(sizes) <= MAX_BATCH
    assert any(B > 128 for B in sizes) and any(64 < B <= 128 for B in sizes), "the reduction wave's second and third term per lane"
    if form == "cols":                                    # every rank sees the whole batch: nothing below applies
        return
    local = [[shard_bounds(B, world, r)[1] - shard_bounds(B, world, r)[0] for r in range(world)] for B in sizes]
    assert all(sum(l) == B for l, B in zip(local, sizes))
    assert any(0 < l[-1] < shard_size(B, world) for l, B in zip(local, sizes)), "no batch has a ragged last shard"
    if world >= 3:
        assert any(l[-1] == 0 for l in local), "no batch leaves a trailing rank empty"
        if world == 4:
            assert local[sizes.index(5)] == [2, 2, 1, 0]
    else:
        assert all(min(l) > 0 for l, B in zip(local, sizes) if B >= 2), "world 2: ceil(B / 2) < B for B >= 2, no rank is empty"
    assert any(shard_size(B, world) % 8 for B in sizes), "every shard is a multiple of k_scatter's 8 slots per workgroup (d = 32)"
    named_u = named_i = hubs_apart = False
    for (u, p, n), B in zip(batches, sizes):
        named_u |= len(_ranks_naming(u, TWICE_USER, B, world)) >= 2
        named_i |= len(_ranks_naming(p, MANY_ITEM, B, world) | _ranks_naming(n, MANY_ITEM, B, world)) >= 2
        ru = _ranks_naming(u, SC.HUB_USER, B, world)
        ri = _ranks_naming(p, SC.HUB_ITEM, B, world) | _ranks_naming(n, SC.HUB_ITEM, B, world)
        hubs_apart |= bool(ru) and bool(ri) and bool(ri - ru)
    assert named_u and named_i, "no row id is named in two ranks' shards, as user and as item"
    if hub > 0:
        assert hubs_apart, "the hub user and the hub item never sit in different ranks' shards"
    for f, v in SPECIALS:                                 # every special row is there
        if f != "pn":
            assert any(({"u": b[0], "p": b[1], "n": b[2]}[f] == v).any() for b in batches), (f, v)
    assert any((b[1] == b[2]).any() for b in batches), "no pos = neg pair"


def _case(mode, d, K, dl, world, form, hub=-1, reg="propagated"):
    return (mode, d, K, dl, hub, reg, world, form, MAX_BATCH)


_MODES_AT = {32: ("fp32", "bf16"), 64: ("fp32", "bf16", "fp8"), 128: ("fp32", "bf16", "fp8"), 256: ("fp32", "bf16", "fp8")}


def _step_cases():
    """(a): five cases per (d, mode) -- K, dense_last, the world and the form cycle at different strides -- + hub + ego."""
    out, i = [], 0
    for d in (32, 64, 128, 256):
        for mode in _MODES_AT[d]:
            for j in range(5):
                K = 1 + (i + j) % 3
                dl = (i // 3 + j // 3 + j) % 2
                out.append(_case(mode, d, K, dl, 2 + (i + 2 * j) % 3, ("rows1", "rows0")[(i + j) % 2]))
            i += 1
    out += [_case("fp32", 32, 2, 0, 3, "rows1", hub=100), _case("bf16", 256, 3, 0, 4, "rows0", hub=100), _case("fp8", 128, 1, 0, 2, "rows1", hub=100),
            _case("fp32", 64, 1, 0, 4, "rows0", hub=100)]
    out += [_case("fp32", 128, 3, 0, 2, "rows0", reg="ego"), _case("bf16", 32, 2, 1, 4, "rows1", reg="ego"), _case("fp8", 256, 1, 0, 3, "rows1", reg="ego")]
    return out


STEP_CASES = _step_cases()

# (b): the C loop.  row_sharded: K = 1, 2, 3 x fp32 / bf16 / fp8, every d, the hub plan; dense: K = 1, ego, every d; rows: every d
LOOP_CASES = [
    _case("fp32", 32, 1, 0, 2, "row_sharded"), _case("bf16", 64, 2, 0, 3, "row_sharded"), _case("fp8", 128, 3, 0, 4, "row_sharded"),
    _case("bf16", 256, 1, 1, 4, "row_sharded"), _case("fp8", 64, 1, 0, 2, "row_sharded"), _case("fp32", 128, 2, 1, 3, "row_sharded"),
    _case("bf16", 32, 3, 1, 2, "row_sharded"), _case("fp8", 256, 2, 0, 3, "row_sharded"), _case("fp32", 64, 3, 0, 4, "row_sharded"),
    _case("bf16", 128, 2, 0, 4, "row_sharded", hub=100), _case("fp32", 32, 1, 0, 3, "row_sharded", hub=100), _case("fp8", 64, 3, 0, 2, "row_sharded", hub=100),
    _case("fp32", 32, 1, 0, 3, "dense"), _case("bf16", 64, 3, 1, 4, "dense"), _case("fp8", 128, 2, 0, 2, "dense"),
    _case("bf16", 256, 1, 0, 2, "dense", reg="ego"), _case("fp32", 128, 2, 0, 4, "dense", hub=100),
    _case("bf16", 32, 2, 0, 4, "rows1"), _case("fp8", 64, 1, 1, 3, "rows1"), _case("fp32", 128, 3, 0, 2, "rows1"),
    _case("bf16", 256, 2, 0, 3, "rows1", hub=100), _case("fp32", 256, 1, 0, 4, "rows1", reg="ego"),
]

# (c): column shards, (W, d) = (2, 128), (2, 256), (4, 256), (4, 128), (8, 256): rank widths 64, 128, 64, 32, 32
COLS_WD = ((2, 128), (2, 256), (4, 256), (4, 128), (8, 256))
COLS_CASES = [_case(("fp32", "bf16")[(i + j) % 2], d, 1 + (i + j) % 3, (i + j // 2) % 2, W, "cols")
              for i, (W, d) in enumerate(COLS_WD) for j in range(4)]
COLS_CASES += [_case("bf16", 256, 2, 0, 2, "cols", hub=100), _case("fp32", 128, 3, 0, 4, "cols", hub=100),
               _case("bf16", 256, 3, 0, 4, "cols", reg="ego"), _case("fp32", 256, 1, 0, 8, "cols", reg="ego")]
COLS_FP8_CASES = [_case("fp8", 128, 2, 0, 2, "cols"), _case("fp8", 256, 3, 1, 2, "cols")]

ALL_CASES = STEP_CASES + LOOP_CASES + COLS_CASES + COLS_FP8_CASES


def pairs(cases, i, j):
    return {(c[i], c[j]) for c in cases}


def check_grids():
    """The coverage the grids are thinned to keep (tests/test_dp_shapes_host.py asserts it again)."""
    S = STEP_CASES
    assert len({case_id(c) for c in ALL_CASES}) == len(ALL_CASES), "two cases share an id"
    assert pairs(S, 1, 0) == {(d, m) for d in _MODES_AT for m in _MODES_AT[d]}, "(d, mode)"
    assert pairs(S, 1, 2) == {(d, K) for d in _MODES_AT for K in (1, 2, 3)}, "(d, K)"
    assert pairs(S, 0, 2) == {(m, K) for m in ("fp32", "bf16", "fp8") for K in (1, 2, 3)}, "(mode, K)"
    assert pairs(S, 2, 3) == {(K, dl) for K in (1, 2, 3) for dl in (0, 1)}, "(K, dense_last)"
    assert pairs(S, 1, 6) == {(d, W) for d in _MODES_AT for W in (2, 3, 4)}, "(d, world)"
    assert pairs(S, 1, 7) == {(d, f) for d in _MODES_AT for f in ("rows0", "rows1")}, "(d, form)"
    assert all(c[3] == 0 for c in ALL_CASES if c[4] > 0)              # the hub plan serves the gathered last layer only
    for mode in ("fp32", "bf16", "fp8"):
        assert any(c[0] == mode and c[4] > 0 for c in S) and any(c[0] == mode and c[5] == "ego" for c in S), mode
    L = LOOP_CASES
    for form in ("rows1", "dense", "row_sharded"):
        assert {c[1] for c in L if c[7] == form} == {32, 64, 128, 256}, form
    rs = [c for c in L if c[7] == "row_sharded"]
    assert pairs(rs, 0, 2) == {(m, K) for m in ("fp32", "bf16", "fp8") for K in (1, 2, 3)} and any(c[4] > 0 for c in rs)
    assert any(c[2] == 1 for c in L if c[7] == "dense") and any(c[5] == "ego" for c in L if c[7] == "dense")
    Cc = COLS_CASES
    assert pairs(Cc, 6, 1) == set(COLS_WD) and {c[1] // c[6] for c in Cc} == {32, 64, 128}
    assert {c[2] for c in Cc} == {1, 2, 3} and {c[0] for c in Cc} == {"fp32", "bf16"} and {c[3] for c in Cc} == {0, 1}
    for W, d in COLS_WD:
        assert {c[0] for c in Cc if (c[6], c[1]) == (W, d)} == {"fp32", "bf16"}, (W, d)
    assert any(c[4] > 0 for c in Cc) and any(c[5] == "ego" for c in Cc)
    assert {(c[6], c[1]) for c in COLS_FP8_CASES} == {(2, 128), (2, 256)}
    assert all(c[0] != "fp8" or c[1] // (c[6] if c[7] == "cols" else 1) >= 64 for c in ALL_CASES)
    assert all(c[6] <= 8 for c in ALL_CASES)


check_grids()
for _c in ALL_CASES:
    check_case(_c)
