"""Host tests of the exact-table restatement of the top-K evaluation sweep (tests/eval_topk_restatement.py): the tables are exact
(fp32 in any order, and the six bf16 product planes of k_eval_topk), the reference ranking is the stable descending sort, every
case exercises the tie rule without letting it excuse a wrong list, and the checker refuses the lists of a kernel that evicts
the first of several equal minima."""
import numpy as np
import pytest
import torch

import eval_topk_restatement as R

FAMILIES = [(4, 0, (32, 64, 128, 256)), (16, 0, (32, 64, 128, 256)), (512, 6, (32, 64))]       # (r, frac_bits, dims)


@pytest.mark.parametrize("r,frac_bits,d", [(r, f, d) for r, f, dims in FAMILIES for d in dims])
def test_exact_table_products_are_exact(r, frac_bits, d):
    """Every user . item product of an exact table: fp32 accumulation in shuffled orders, and the six product planes of split3
    (hh, hm, mh, hl, lh, mm; the l plane is zero, so the three planes the kernel drops vanish), equal the float64 product bit
    for bit."""
    rng = np.random.Generator(np.random.PCG64([r, d]))
    n_users, m_items = 12, 96
    E = R.exact_table(n_users, m_items, d, r, frac_bits, rng)
    assert E.dtype == np.float32 and E.shape == (n_users + m_items, d)
    q = E.astype(np.float64) * 2.0 ** frac_bits
    assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= r
    assert np.abs(q).max() > r // 2                                        # the range is used
    U, I = E[:n_users], E[n_users:]
    want = U.astype(np.float64) @ I.astype(np.float64).T
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    for trial in range(4):
        order = np.arange(d) if trial == 0 else rng.permutation(d)
        acc = np.zeros((n_users, m_items), np.float32)
        for k in order:
            prod = U[:, k, None] * I[None, :, k]
            assert prod.dtype == np.float32
            acc = acc + prod
            assert acc.dtype == np.float32
        assert np.array_equal(acc.astype(np.float64), want), trial
    uh, um, ul = R.split3(U)
    ih, im, il = R.split3(I)
    for x, (h, m, l) in ((U, (uh, um, ul)), (I, (ih, im, il))):
        assert not l.any()                                                  # at most 16 significant bits
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64), x.astype(np.float64))
        for p in (h, m):                                                    # bf16 values
            assert not (p.view(np.uint32) & np.uint32(0xffff)).any()
    if r >= 256:
        assert um.any() and im.any()                                        # the m plane carries bits
    else:
        assert not um.any() and not im.any()                                # one plane
    acc = np.zeros((n_users, m_items), np.float32)
    for a, b in ((im, um), (ih, ul), (il, uh), (ih, um), (im, uh), (ih, uh)):      # the kernel's order: smallest planes first
        for k in range(d):
            acc = acc + a[None, :, k] * b[:, k, None]
    assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), want)


def test_split3_is_the_kernels_split():
    """On arbitrary fp32 values: three bf16 values that sum to x exactly."""
    rng = np.random.Generator(np.random.PCG64(3))
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(np.float32)
    h, m, l = R.split3(x)
    for p in (h, m):
        assert not (p.view(np.uint32) & np.uint32(0xffff)).any()
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    assert (np.abs(l.astype(np.float64)) <= np.abs(x.astype(np.float64)) * 2.0 ** -14).all()


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_reference_is_the_stable_sort_and_case_conditions(c):
    """rank_reference against torch.sort(descending, stable) on the same float64 matrix, and the two conditions every case must
    fulfil, from the reference alone: >= 85 % of the (slot, rank) pairs lie strictly above the cut score (the loose rule at the
    cut cannot excuse a wrong list) and >= 10 % of the slots have a tie group that straddles the cut (the tie rule is
    exercised)."""
    p, ref = R.case_reference(c)
    assert c.d * c.r ** 2 <= 2 ** 24
    n = len(p.users)
    assert n == c.n_eval and ref.ids.shape == (n, c.K)
    if n > 4:
        assert len(np.unique(p.users)) < n and not np.array_equal(p.users, np.sort(p.users))       # repeats, unsorted
    S = torch.from_numpy(ref.scores)
    val, idx = torch.sort(S, dim=1, descending=True, stable=True)
    assert np.array_equal(idx[:, :c.K].numpy(), ref.ids)
    assert np.array_equal(val[:, :c.K].numpy(), ref.top)
    assert np.array_equal(val[:, c.K - 1].numpy(), ref.cut)
    if c.m_items > c.K:
        assert np.array_equal((val[:, c.K] == val[:, c.K - 1]).numpy(), ref.straddle)
    for s in range(0, n, max(1, n // 7)):
        assert np.array_equal(ref.group[s], np.flatnonzero(ref.scores[s] == ref.cut[s]))
    above = float((ref.top > ref.cut[:, None]).mean())
    straddle = float(ref.straddle.mean())
    print(f"{R.case_id(c)}: pairs strictly above the cut {above:.3f}, slots with a straddling tie {straddle:.3f}")
    assert above >= 0.85, above
    assert straddle >= 0.10, straddle


def test_case_list_covers_the_dispatch():
    """The case list holds both sides of the two 16-bit-id boundaries, every d, K on both sides of 20 and 64, and user lists of
    1, 127, 128 and 129 slots."""
    have = {(c.m_items, c.d, c.K) for c in R.CASES}
    for want in [(1000, 32, 7), (4095, 64, 20), (3000, 128, 50), (3000, 256, 64), (4095, 256, 20), (4096, 32, 20), (10007, 64, 20),
                 (196416, 64, 20), (196417, 64, 20), (10007, 64, 50), (130944, 32, 64), (130945, 32, 64), (10007, 128, 20),
                 (10007, 128, 50), (10007, 256, 20), (10007, 256, 64), (300, 32, 256), (3001, 64, 65), (10007, 128, 128),
                 (10007, 256, 256)]:
        assert want in have, want
    assert {1, 127, 128, 129} <= {c.n_eval for c in R.CASES}
    assert all(c.n_eval <= 160 for c in R.CASES)
    assert any(c.r == 512 for c in R.CASES)


def _emulated_lists(c, slots):
    p, ref = R.case_reference(c)
    ids = ref.ids.copy()
    for s in slots:
        ids[s] = R.emulate_first_minimum(ref.scores[s], c.K)
    return ref, ids


def test_checker_refuses_first_minimum_eviction():
    """A list that replaces the first of several equal minima keeps the wrong members of the cut tie group (K = 2, scores
    1, 1, 5: ids [2, 1], not [2, 0]).  Its lists pass the loose rule -- they hold the right scores, sorted -- and fail the
    strict one: the checker tells the two apart."""
    assert R.emulate_first_minimum(np.array([1.0, 1.0, 5.0]), 2).tolist() == [2, 1]
    c = next(c for c in R.CASES if (c.m_items, c.d, c.K, c.r) == (3000, 32, 20, 4))
    ref, ids = _emulated_lists(c, range(c.n_eval))
    wrong = int((ids != ref.ids).any(axis=1).sum())
    print(f"first-minimum eviction deviates from (score, id) in {wrong} of {c.n_eval} slots")
    assert wrong >= c.n_eval // 10
    sc = np.take_along_axis(ref.scores, ids, axis=1).astype(np.float32)
    R.check_lists(ref, ids, sc, strict=False)
    with pytest.raises(AssertionError, match="lowest ids"):
        R.check_lists(ref, ids, sc, strict=True)
    R.check_lists(ref, ref.ids, ref.top.astype(np.float32), strict=True)


def test_checker_refuses_other_wrong_lists():
    """One defect at a time on the reference's own lists: a wrong id above the cut, a foreign score, an id twice, an id out of
    range, equal scores in the wrong id order, a reported score that is not the item's, a stranger at the cut."""
    c = next(c for c in R.CASES if (c.m_items, c.d, c.K, c.r) == (3000, 32, 20, 4))
    p, ref = R.case_reference(c)
    good_sc = ref.top.astype(np.float32)
    s = int(np.flatnonzero(ref.straddle & (ref.top[:, 0] > ref.top[:, 1]))[0])

    def refused(ids, sc=None, strict=False):
        with pytest.raises(AssertionError):
            R.check_lists(ref, ids, good_sc if sc is None else sc, strict=strict)

    ids = ref.ids.copy(); ids[s, [0, 1]] = ids[s, [1, 0]]; refused(ids)                  # order above the cut
    ids = ref.ids.copy(); ids[s, 0] = int(np.argmin(ref.scores[s])); refused(ids)        # a low scorer in first place
    ids = ref.ids.copy(); ids[s, 1] = ids[s, 0]; refused(ids)                            # an id twice
    ids = ref.ids.copy(); ids[s, 0] = c.m_items; refused(ids)                            # out of range
    ids = ref.ids.copy(); ids[s, 0] = -1; refused(ids)
    sc = good_sc.copy(); sc[s, 3] = np.nextafter(sc[s, 3], np.float32(np.inf)); refused(ref.ids, sc)       # one ulp off
    tie = np.flatnonzero(ref.top[s, 1:] == ref.top[s, :-1])
    if len(tie):
        ids = ref.ids.copy(); k = int(tie[0]); ids[s, [k, k + 1]] = ids[s, [k + 1, k]]; refused(ids)        # ties out of id order
    # another member of the cut tie group in the last place: fine under the loose rule, refused under the strict one
    other = [g for g in ref.group[s] if g not in ref.ids[s]]
    ids = ref.ids.copy(); ids[s, -1] = other[-1]
    R.check_lists(ref, ids, good_sc, strict=False)
    refused(ids, strict=True)
    # an item from below the cut in the last place
    below = int(np.flatnonzero(ref.scores[s] < ref.cut[s])[0])
    ids = ref.ids.copy(); ids[s, -1] = below; refused(ids)
