"""The top-K evaluation sweep on tables whose scores are exact (tests/eval_topk_restatement.py): every form of the dispatch in
eval_topk / eval_topk_big, through lgcn_eval_topk, _masked, _fp32 and lgcn_eval_topk_ex, against the float64 ranking by
(score descending, id ascending) with NO tolerance -- scores bit for bit, ids rank by rank above the cut score, the cut tie
group represented by distinct members of it in id order (which members is unspecified: eval_topk_restatement.strict_rule).
Then the edges: catalogues of 1 .. 64 items and m_items == K, users positive on (nearly) every item, real scores
below the -1024 of a train positive, an all-zero user row, a constant table, NULL scores, guard elements around the outputs."""
import numpy as np
import pytest
import torch

import eval_topk_restatement as R

DEV = "cuda:0"
gpu = pytest.mark.gpu
GUARD = 64                        # elements before and after each output that must stay as they were


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Problem:
    """A problem on the device: table, user list, train CSR, masks (built once)."""

    def __init__(self, pkg, E, n_users, users, rows):
        self.pkg, self.n_users, self.m_items, self.d = pkg, n_users, E.shape[0] - n_users, E.shape[1]
        self.n = len(users)
        ptr, idx = R.csr(rows)
        self.E, self.users, self.ptr, self.idx = _dev(E), _dev(users.astype(np.int32)), _dev(ptr), _dev(idx)
        L, lib = pkg._lib, pkg._lib.load()
        self.masks = torch.empty(int(lib.lgcn_eval_mask_words(self.m_items, self.n)), dtype=torch.int32, device=DEV)
        L.check(lib.lgcn_eval_build_masks(L.tp(self.users), self.n, L.tp(self.ptr), L.tp(self.idx), self.m_items, L.tp(self.masks),
                                          L.current_stream()), "lgcn_eval_build_masks")

    def entries(self, K):
        """(name, entry, masks?, fp32?) of every way to the sweep at this K."""
        ex = [("ex", "ex", False, False), ("ex+masks", "ex", True, False), ("ex fp32", "ex", False, True),
              ("ex fp32+masks", "ex", True, True)]
        if K > 64:
            return ex
        return [("topk", "topk", False, False), ("masked", "masked", True, False), ("fp32", "fp32", False, True)] + ex

    def run(self, K, entry, masks=False, fp32=False, scores=True):
        """-> ids [n, K] int32, scores [n, K] fp32 or None (numpy); asserts rc == 0 and that the guards are untouched."""
        L, lib = self.pkg._lib, self.pkg._lib.load()
        n = self.n
        ibuf = torch.full((n * K + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
        sbuf = torch.full((n * K + 2 * GUARD,), 7.0, dtype=torch.float32, device=DEV)
        out_i, out_s = ibuf[GUARD:GUARD + n * K], (sbuf[GUARD:GUARD + n * K] if scores else None)
        head = (L.tp(self.E), self.n_users, self.m_items, self.d, L.tp(self.users), n, L.tp(self.ptr), L.tp(self.idx))
        st = L.current_stream()
        if entry == "topk":
            rc = lib.lgcn_eval_topk(*head, K, L.tp(out_i), L.tp(out_s), st)
        elif entry == "masked":
            rc = lib.lgcn_eval_topk_masked(*head, K, L.tp(out_i), L.tp(out_s), L.tp(self.masks), st)
        elif entry == "fp32":
            rc = lib.lgcn_eval_topk_fp32(*head, K, L.tp(out_i), L.tp(out_s), st)
        else:
            rc = lib.lgcn_eval_topk_ex(*head, L.tp(self.masks if masks else None), K, L.tp(out_i), L.tp(out_s), n * K,
                                       L.EVAL_FP32 if fp32 else 0, st)
        torch.cuda.synchronize()
        assert rc == 0, (entry, lib.lgcn_last_error())
        for buf, fill in ((ibuf, -7), (sbuf, 7.0)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n * K:] == fill).all()), (entry, "a guard element was written")
        if not scores:
            assert bool((sbuf == 7.0).all())
        return out_i.view(n, K).cpu().numpy(), (out_s.view(n, K).cpu().numpy() if scores else None)


def _check_every_entry(prob, ref, K, what):
    """Every entry point against the reference; all of them the same scores bitwise and, outside the cut tie group, the same
    ids; one of them once more without scores.  -> the first entry's ids."""
    strict = R.strict_rule(prob.m_items)
    first = None
    for name, entry, masks, fp32 in prob.entries(K):
        ids, sc = prob.run(K, entry, masks, fp32)
        R.check_lists(ref, ids, sc, strict, (what, name))
        print(f"{what} {name}: {int((ids != ref.ids).any(axis=1).sum())} of {len(ids)} lists keep other members of the cut tie group than the lowest ids")
        if first is None:
            first = (ids, sc)
        else:
            assert np.array_equal(sc, first[1]), (what, name, "scores differ between entry points")
            R.check_same_outside_cut(ref, ids, first[0], (what, name))
    name, entry, masks, fp32 = prob.entries(K)[0]
    ids, sc = prob.run(K, entry, masks, fp32, scores=False)               # topk_scores == NULL
    assert sc is None
    R.check_lists(ref, ids, None, strict, (what, name, "no scores"))
    return first[0]


@gpu
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_eval_topk_exact_every_form(pkg, c):
    """One case per form of the dispatch (the form is in the case), bit for bit."""
    p, ref = R.case_reference(c)
    prob = _Problem(pkg, p.E, p.n_users, p.users, p.rows)
    ids = _check_every_entry(prob, ref, c.K, c.form)
    if (c.m_items, c.d, c.K, c.r) == (3000, 32, 20, 4):        # a measurement, no assertion: is the emulation of the list right?
        emu = np.stack([R.emulate_first_minimum(ref.scores[s], c.K) for s in range(c.n_eval)])
        print(f"{c.form}: {int((emu == ids).all(axis=1).sum())} of {c.n_eval} lists are those of emulate_first_minimum")


def _edge_problem(m_items, d, K, seed):
    """r = 16 table (at d >= 64 many real scores lie below -1024) with user 0 an all-zero row (every score 0), user 1 positive
    on every item, user 2 on all but K - 3 items, user 3 on all but K + 5 (the list's end falls among real scores, some of them
    below -1024: those rank under the train positives); the others as the cases build them."""
    rng = np.random.Generator(np.random.PCG64([m_items, d, K, seed]))
    n_users = 40
    E = R.exact_table(n_users, m_items, d, 16, 0, rng)
    E[0] = 0.0
    rows = R.train_lists(rng, n_users, m_items)
    rows[0] = rows[0][::2].copy()
    rows[1] = np.arange(m_items, dtype=np.int32)
    for u, free in ((2, K - 3), (3, K + 5), (4, K - 3)):
        if 0 <= free <= m_items:
            keep = rng.choice(m_items, free, replace=False)
            rows[u] = np.setdiff1d(np.arange(m_items), keep).astype(np.int32)
    users = np.concatenate([np.array([3, 1, 0, 2, 1, 4, 0], np.int32), rng.integers(0, n_users, 30).astype(np.int32)])
    return E, n_users, users, rows


@gpu
@pytest.mark.parametrize("m_items,K", [(1, 1), (31, 7), (31, 31), (32, 20), (32, 32), (33, 20), (33, 33), (64, 20), (64, 64),
                                       (20, 20), (65, 65), (256, 256), (257, 256)])
@pytest.mark.parametrize("d", [32, 64])
def test_eval_topk_exact_tiny_catalogues(pkg, m_items, K, d):
    """Catalogues of one tile or two, a last tile of 1, 31, 32 and 33 rows, and m_items == K (every item returned: real scores
    below -1024 after the train positives at -1024, rows past the table never)."""
    E, n_users, users, rows = _edge_problem(m_items, d, K, 0)
    ref = R.rank_reference(E, n_users, users, rows, K)
    if m_items == K:
        assert np.array_equal(np.sort(ref.ids, axis=1), np.tile(np.arange(K), (len(users), 1)))
        if d == 64 and K >= 64:
            assert (ref.top < R.MASKED).any()                           # a real score below a train positive's
    _check_every_entry(_Problem(pkg, E, n_users, users, rows), ref, K, ("tiny", m_items, K, d))


@gpu
@pytest.mark.parametrize("m_items", [1000, 4100])
@pytest.mark.parametrize("K", [7, 20, 64, 200])
@pytest.mark.parametrize("d", [64, 256])
def test_eval_topk_exact_minus_1024_tail(pkg, m_items, K, d):
    """Users positive on every item and on all but K - 3: the unmasked items scoring above -1024 first, then train positives at
    exactly -1024.0 (which positives: unspecified, they tie) and never an unmasked item scoring below -1024 while a positive is
    left.  The all-zero user: every unmasked item at 0, so any K of them in id order.  With and
    without masks, split product and fp32 instructions (every entry point)."""
    E, n_users, users, rows = _edge_problem(m_items, d, K, 1)
    ref = R.rank_reference(E, n_users, users, rows, K)
    strict = R.strict_rule(m_items)
    # the reference itself shows the edge (from the reference alone)
    s1, s0, s2, s3 = 1, 2, 3, 0                                          # slots of users 1, 0, 2, 3
    assert (ref.top[s1] == R.MASKED).all() and np.array_equal(ref.ids[s1], np.arange(K))
    free0 = np.setdiff1d(np.arange(m_items), rows[0])
    assert (ref.top[s0] == 0.0).all() and np.array_equal(ref.ids[s0], free0[:K])
    n_tail2 = int((ref.top[s2] == R.MASKED).sum())
    assert n_tail2 >= 3 and (ref.top[s2, K - n_tail2:] == R.MASKED).all()
    assert np.array_equal(ref.ids[s2, K - n_tail2:], rows[2][:n_tail2])
    free3 = np.setdiff1d(np.arange(m_items), rows[3])
    low3 = free3[ref.scores[s3, free3] < R.MASKED]
    assert not np.isin(low3, ref.ids[s3]).any()
    prob = _Problem(pkg, E, n_users, users, rows)
    for name, entry, masks, fp32 in prob.entries(K):
        ids, sc = prob.run(K, entry, masks, fp32)
        R.check_lists(ref, ids, sc, strict, ("tail", name))
        assert (sc[s1] == np.float32(-1024.0)).all() and np.isin(ids[s1], rows[1]).all()
        assert (sc[s2, K - n_tail2:] == np.float32(-1024.0)).all() and np.isin(ids[s2, K - n_tail2:], rows[2]).all()
        assert not np.isin(low3, ids[s3]).any()
        if strict:
            assert np.array_equal(ids[s1], np.arange(K)) and np.array_equal(ids[s0], free0[:K])
            assert np.array_equal(ids[s2, K - n_tail2:], rows[2][:n_tail2])


@gpu
@pytest.mark.parametrize("m_items,d,K", [(100, 32, 20), (3000, 64, 20), (3000, 256, 64), (3000, 128, 200), (5000, 64, 20), (5000, 32, 64),
                                         (5000, 128, 100)])
def test_eval_topk_exact_constant_table(pkg, m_items, d, K):
    """Every entry 0.5: every score d / 4, the whole catalogue one tie.  K distinct items that are no train positives, in id
    order (the reference's are 0, 1, 2, ... skipping the positives; which ones the sweep keeps is unspecified); positives follow
    at -1024 only for the users with fewer than K other items."""
    n_users = 40
    rng = np.random.Generator(np.random.PCG64([m_items, d, K]))
    E = np.full((n_users + m_items, d), 0.5, np.float32)
    rows = R.train_lists(rng, n_users, m_items)
    rows[1] = np.arange(m_items, dtype=np.int32)
    rows[2] = np.setdiff1d(np.arange(m_items), rng.choice(m_items, K - 3, replace=False)).astype(np.int32)
    users = np.concatenate([np.array([2, 1, 5, 1], np.int32), rng.integers(0, n_users, 36).astype(np.int32)])
    ref = R.rank_reference(E, n_users, users, rows, K)
    for s, u in enumerate(users.tolist()):
        free = np.setdiff1d(np.arange(m_items), rows[u])
        want = np.concatenate([free, rows[u]])[:K]
        assert np.array_equal(ref.ids[s], want)
        assert (ref.top[s, :min(K, len(free))] == d / 4).all() and (ref.top[s, len(free):] == R.MASKED).all()
    _check_every_entry(_Problem(pkg, E, n_users, users, rows), ref, K, ("constant", m_items, d, K))
