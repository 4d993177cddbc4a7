"""The grid of tests/dp_cases.py, judged on the CPU: what tests/test_gpu_dp_shapes.py relies on when it calls a case covered.
Every condition dp_cases asserts at import is asserted again here against the package's own parallel.shard_bounds, so a batch
size or a world changed in the grid fails HERE and cannot quietly make a GPU case vacuous; parallel.row_ranges, column_range and
block_numel are pinned on the 300 x 600 graph the GPU cases run on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dp_cases as D                               # noqa: E402
import storage_cases as SC                         # noqa: E402
from storage_cases import storage_graph            # noqa: E402,F401  (fixture: the graph, written once per session)

_CACHE = {}


def _adj(pkg, path):
    if "adj" not in _CACHE:
        try:
            ds, _ = SC.make_model(pkg, ("fp32", 32, 1, 0, -1, "propagated"), path)
            _CACHE["adj"] = ds.getSparseGraphCSR()
        finally:
            pkg.world.configure([])
    return _CACHE["adj"]


def test_grids_keep_their_coverage():
    D.check_grids()
    assert 55 <= len(D.STEP_CASES) <= 70
    assert D.BATCH_SIZES == (300, 65, 37, 5, 1) and D.MAX_BATCH == 300


def test_shard_arithmetic_is_the_package_s(pkg):
    par = pkg.parallel
    for B in list(D.BATCH_SIZES) + [2, 3, 4, 64, 128, 129]:
        for W in (1, 2, 3, 4, 8):
            assert D.shard_size(B, W) == par.shard_size(B, W)
            for r in range(W):
                assert D.shard_bounds(B, W, r) == par.shard_bounds(B, W, r)
    got = {W: [par.shard_size(B, W) for B in D.BATCH_SIZES] for W in (2, 3, 4)}
    assert got == {2: [150, 33, 19, 3, 1], 3: [100, 22, 13, 2, 1], 4: [75, 17, 10, 2, 1]}
    assert [par.shard_bounds(5, 4, r) for r in range(4)] == [(0, 2), (2, 4), (4, 5), (5, 5)]          # rank 3 gets nothing
    for B in range(2, 301):                                                                             # world 2: no empty rank for B >= 2
        assert par.shard_bounds(B, 2, 1)[1] > par.shard_bounds(B, 2, 1)[0]
    assert par.shard_bounds(1, 2, 1) == (1, 1)                                                          # (B = 1 does leave rank 1 empty)


@pytest.mark.parametrize("case", D.ALL_CASES, ids=D.case_id)
def test_case_conditions(pkg, case):
    """dp_cases.check_case on the batches, and the same conditions recomputed from parallel.shard_bounds."""
    par = pkg.parallel
    batches = D.make_batches(case)
    again = D.make_batches(case)
    assert all(np.array_equal(a, b) for x, y in zip(batches, again) for a, b in zip(x, y))           # the batches are a function of the case
    D.check_case(case, batches)
    world, form, hub = case[6], case[7], case[4]
    for u, p, n in batches:
        assert u.min() >= 0 and u.max() < SC.N_USERS and min(p.min(), n.min()) >= 0 and max(p.max(), n.max()) < SC.M_ITEMS
        assert not (p == SC.BIG_ITEM).any() and not (n == SC.BIG_ITEM).any() and not (p == SC.ISOLATED_ITEM).any()
    if form == "cols":
        return
    sizes = [len(b[0]) for b in batches]
    local = [[par.shard_bounds(B, world, r)[1] - par.shard_bounds(B, world, r)[0] for r in range(world)] for B in sizes]
    assert any(0 < l[-1] < par.shard_size(B, world) for l, B in zip(local, sizes))
    assert any(l[-1] == 0 for l in local) if world >= 3 else all(min(l) > 0 for l, B in zip(local, sizes) if B >= 2)
    assert any(par.shard_size(B, world) % 8 for B in sizes) and any(par.shard_size(B, world) % 4 for B in sizes)
    assert max(sizes) > 128 and sorted(sizes)[-2] > 64

    def ranks(arr, v, B):
        return {r for r in range(world) if (arr[slice(*par.shard_bounds(B, world, r))] == v).any()}
    big = [(b, B) for b, B in zip(batches, sizes) if B >= D.MIN_SPECIAL_BATCH]
    assert len(big) == 3
    for (u, p, n), B in big:                                # in EVERY batch that carries the specials
        assert len(ranks(u, D.TWICE_USER, B)) >= 2 and len(ranks(p, D.MANY_ITEM, B)) == world
        ru, rp, rn = ranks(u, SC.HUB_USER, B), ranks(p, SC.HUB_ITEM, B), ranks(n, SC.HUB_ITEM, B)
        assert ru == {0} and 1 in rp and (2 % world) in rn, (ru, rp, rn)
        if hub > 0:
            assert (rp | rn) - ru
        assert (n == SC.ISOLATED_ITEM).any() and (u == SC.N_USERS - 1).any() and (p == SC.M_ITEMS - 1).any() and (p == n).any()
        for f, v in D.SPECIALS:                             # no special was overwritten by a later one
            if f != "pn":
                assert ({"u": u, "p": p, "n": n}[f] == v).any(), (f, v)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_row_ranges_on_the_case_graph(pkg, storage_graph, world):
    par, adj = pkg.parallel, _adj(pkg, storage_graph)
    N = SC.N_USERS + SC.M_ITEMS
    assert adj.shape[0] == N
    rr = par.row_ranges(adj.indptr, SC.N_USERS, world)
    assert rr.shape == (world, 4)
    assert (rr[:, 1] > rr[:, 0]).all() and (rr[:, 3] > rr[:, 2]).all()                       # every rank owns a user row and an item row
    assert rr[0, 0] == 0 and rr[-1, 1] == SC.N_USERS and rr[0, 2] == SC.N_USERS and rr[-1, 3] == N
    assert (rr[1:, 0] == rr[:-1, 1]).all() and (rr[1:, 2] == rr[:-1, 3]).all()               # the ranges tile [0, N) exactly
    owned = np.concatenate([par.owned_rows(rr, r) for r in range(world)])
    assert np.array_equal(np.sort(owned), np.arange(N))
    iso = SC.N_USERS + SC.ISOLATED_ITEM
    assert adj.indptr[iso + 1] == adj.indptr[iso]
    assert sum(int(iso in set(par.owned_rows(rr, r).tolist())) for r in range(world)) == 1   # the empty row has an owner


def test_hub_rows_have_different_owners(pkg, storage_graph):
    """The hub user and the hub item are row 0 of their blocks, and parallel.row_ranges gives row 0 of either block to rank 0 at
    every world size: under ITS table the two hub rows can never have different owners on this graph (pinned here, so that the
    statement stays true).  The row-sharded hub cases therefore run on dp_cases.rotate_item_ranges of that table -- as good a
    tiling -- under which rank 0 owns the hub user and rank 1 the hub item, at every world size."""
    par, adj = pkg.parallel, _adj(pkg, storage_graph)
    N = SC.N_USERS + SC.M_ITEMS
    deg = np.diff(adj.indptr)
    assert sorted(np.flatnonzero(deg > 100).tolist()) == [SC.HUB_USER, SC.N_USERS + SC.HUB_ITEM]      # hub_nnz = 100: these two rows
    for world in (2, 3, 4):
        rr = par.row_ranges(adj.indptr, SC.N_USERS, world)
        own = lambda t, row: [r for r in range(world) if row in set(par.owned_rows(t, r).tolist())]      # noqa: E731
        assert own(rr, SC.HUB_USER) == [0] and own(rr, SC.N_USERS + SC.HUB_ITEM) == [0]
        rot = D.rotate_item_ranges(rr)
        assert own(rot, SC.HUB_USER) == [0] and own(rot, SC.N_USERS + SC.HUB_ITEM) == [1]
        assert np.array_equal(np.sort(np.concatenate([par.owned_rows(rot, r) for r in range(world)])), np.arange(N))
        assert (rot[:, 1] > rot[:, 0]).all() and (rot[:, 3] > rot[:, 2]).all() and np.array_equal(rot[:, :2], rr[:, :2])
        assert len(own(rot, SC.N_USERS + SC.ISOLATED_ITEM)) == 1
    assert any(c[7] == "row_sharded" and c[4] > 0 for c in D.LOOP_CASES)


def test_column_range_and_block_numel(pkg):
    par = pkg.parallel
    for W, d in D.COLS_WD + ((2, 64), (1, 256)):
        cuts = [par.column_range(d, W, r) for r in range(W)]
        assert cuts[0][0] == 0 and cuts[-1][1] == d and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert all(hi - lo == d // W for lo, hi in cuts)
    assert sorted(d // W for W, d in D.COLS_WD) == [32, 32, 64, 64, 128]
    for bad in ((3, 128), (8, 128), (2, 32)):
        with pytest.raises(ValueError):
            par.column_range(bad[1], bad[0], 0)
    for B in D.BATCH_SIZES:
        for W in (2, 3, 4):
            for d in (32, 64, 128, 256):
                S = par.shard_size(B, W)
                assert par.block_numel(B, W, d) == 3 * S * d + 2 * S
