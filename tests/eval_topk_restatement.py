"""The top-K evaluation sweep (k_eval_topk, csrc/lgcn_eval.hip) restated in numpy on tables whose scores are EXACT, so that
the GPU lists can be compared with no tolerance at all, ties included.  numpy only: imported by the host tests
(test_eval_topk_restatement.py) and by the GPU tests (test_gpu_eval_topk_exact.py).

exact_table     fp32 tables of small integers (times a power of two): every dot product is exact in fp32 in any summation order
                and in the split-bf16 product of the kernel.
split3          the kernel's split of an fp32 value into three bf16 planes.
rank_reference  float64 scores, train positives at -1024, ordered by (score descending, id ascending); the cut score and the
                cut tie group of every slot.
check_lists     the contract of lgcn_eval_topk / _ex asserted on a result.
emulate_first_minimum   the kernel's list as read from its code: sequential arrival, replace the FIRST slot holding the minimum.
                It keeps other members of the cut tie group than the lowest ids: the strict rule of the checker refuses it,
                the loose one (the documented contract) accepts it.
CASES           one case per form of the dispatch in eval_topk / eval_topk_big."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

MASKED = -1024.0                  # Procedure.py:181: rating[train positives] = -(1 << 10)


def strict_rule(m_items):
    """Whether the cut tie group must be represented by its lowest ids at this catalogue size.  The header promises, for every
    size, only that the members returned are distinct members of the group: k_eval_topk replaces the first slot holding the
    minimum, which on a 4095 x 64 table at K = 20 kept other members in 31 of 127 lists (MI355X), and the (score, id) key that
    would keep the lowest ids costs 3-13 % of the sweep (profiles/eval_topk_exact)."""
    return False


def exact_table(n_users, m_items, d, r, frac_bits, rng):
    """fp32 [n_users + m_items, d] with entries i * 2**-frac_bits, i an integer in [-r, r].  Every product of two entries is an
    integer below r**2 (times 2**-2 frac_bits) and every partial sum of a row product stays below d * r**2 <= 2**24: exact in
    fp32 whatever the order.  r < 2**16 keeps an entry within 16 significant bits: the third bf16 plane of split3 is zero."""
    assert d * r * r <= 2 ** 24 and r < 2 ** 16, (d, r)
    i = rng.integers(-r, r + 1, (n_users + m_items, d))
    return (i.astype(np.float64) * 2.0 ** -frac_bits).astype(np.float32)


def split3(x):
    """x (fp32) -> h, m, l (fp32 arrays whose values are bf16): h = x with the low 16 bits cleared, m = (x - h) likewise,
    l = x - h - m (k_eval_topk's split3: truncation, every subtraction exact)."""
    x = np.ascontiguousarray(x, np.float32)
    mask = np.uint32(0xffff0000)
    h = (x.view(np.uint32) & mask).view(np.float32)
    r = (x - h).astype(np.float32)
    m = (r.view(np.uint32) & mask).view(np.float32)
    l = (r - m).astype(np.float32)
    return h, m, l


def scores64(E, n_users, users, train_rows):
    """float64 [n_eval, m_items]: U . I^T with the train positives of every slot's user at -1024."""
    E = np.asarray(E, np.float64)
    users = np.asarray(users, np.int64)
    S = E[:n_users][users] @ E[n_users:].T
    for s, u in enumerate(users.tolist()):
        if len(train_rows[u]):
            S[s, np.asarray(train_rows[u], np.int64)] = MASKED
    return S


Reference = namedtuple("Reference", "scores ids top cut group straddle K m_items")
# scores [n, m] float64 (masked); ids / top [n, K]: the ranked ids and their scores; cut [n]: the K-th score; group: per slot the
# ascending ids of ALL items scoring exactly cut; straddle [n] bool: the score at rank K + 1 equals the cut.


def rank_reference(E, n_users, users, train_rows, K):
    S = scores64(E, n_users, users, train_rows)
    n, m = S.shape
    assert 1 <= K <= m
    ids = np.empty((n, K), np.int64)
    top = np.empty((n, K), np.float64)
    cut = np.empty(n, np.float64)
    straddle = np.zeros(n, bool)
    group = []
    for s in range(n):
        row = S[s]
        kth = np.partition(row, m - K)[m - K]                 # the K-th largest value
        cand = np.flatnonzero(row >= kth)                     # ascending ids: everything that can be in the list
        order = np.lexsort((cand, -row[cand]))[:K]            # score descending, then id ascending
        ids[s] = cand[order]
        top[s] = row[ids[s]]
        cut[s] = kth
        g = np.flatnonzero(row == kth)
        group.append(g)
        straddle[s] = (row > kth).sum() + len(g) > K
    return Reference(S, ids, top, cut, group, straddle, K, m)


def check_lists(ref, got_ids, got_scores, strict, what=""):
    """The contract on one result (got_ids [n, K] integers, got_scores [n, K] fp32 or None).  No tolerance anywhere.
    strict: the cut tie group is represented by its lowest ids, so the whole list is the reference's; otherwise any distinct
    members of the group."""
    got_ids = np.asarray(got_ids).astype(np.int64)
    n, K = ref.ids.shape
    assert got_ids.shape == (n, K), (what, got_ids.shape)
    assert got_ids.min() >= 0 and got_ids.max() < ref.m_items, (what, "id out of range", int(got_ids.min()), int(got_ids.max()))
    srt = np.sort(got_ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "an id twice in one list", np.argwhere(srt[:, 1:] == srt[:, :-1])[:4].tolist())
    own = np.take_along_axis(ref.scores, got_ids, axis=1)                   # the float64 score of every returned id
    if got_scores is not None:
        got_scores = np.asarray(got_scores)
        assert got_scores.dtype == np.float32 and got_scores.shape == (n, K)
        bad = got_scores.astype(np.float64) != own
        assert not bad.any(), (what, "a reported score is not its item's score", np.argwhere(bad)[:4].tolist())
    # rank by rank the reference's score: with both lists sorted this is the equality of the slot's multiset of scores
    bad = own != ref.top
    assert not bad.any(), (what, "scores differ from the reference's", np.argwhere(bad)[:4].tolist(),
                           own[bad][:4].tolist(), ref.top[bad][:4].tolist())
    # (score descending, id ascending)
    bad = (own[:, 1:] == own[:, :-1]) & (got_ids[:, 1:] < got_ids[:, :-1])
    assert not bad.any(), (what, "equal scores not in id order", np.argwhere(bad)[:4].tolist())
    above = ref.top > ref.cut[:, None]
    bad = above & (got_ids != ref.ids)
    assert not bad.any(), (what, "wrong id above the cut", np.argwhere(bad)[:4].tolist())
    # at the cut: members of the tie group (their score is the cut score: checked above), distinct (checked above)
    if strict:
        bad = got_ids != ref.ids
        assert not bad.any(), (what, "the cut tie group is not represented by its lowest ids", int(bad.any(axis=1).sum()), "slots",
                               np.argwhere(bad)[:4].tolist(), got_ids[bad][:4].tolist(), ref.ids[bad][:4].tolist())


def check_same_outside_cut(ref, ids_a, ids_b, what=""):
    """Two entry points on one problem: the same ids wherever the score lies strictly above the cut."""
    above = ref.top > ref.cut[:, None]
    a, b = np.asarray(ids_a).astype(np.int64), np.asarray(ids_b).astype(np.int64)
    bad = above & (a != b)
    assert not bad.any(), (what, np.argwhere(bad)[:4].tolist())


def emulate_first_minimum(scores, K):
    """One slot's list as k_eval_topk keeps it where one workgroup sweeps the catalogue: items arrive tile by tile (32 rows), inside a
    tile the lower lane's rows (0-3, 8-11, ...) before the upper lane's (4-7, 12-15, ...); a score enters when it is strictly
    above the list's minimum and replaces the FIRST slot holding that minimum; the list is sorted by (score descending, id
    ascending) at the end.  -> ids [K]."""
    m = len(scores)
    ls = np.full(K, -np.inf)
    li = np.full(K, -1, np.int64)
    lane_rows = [r for h in (0, 1) for r in range(32) if (r >> 2) % 2 == h]
    pmin, thr = 0, -np.inf
    for base in range(0, m, 32):
        for r in lane_rows:
            i = base + r
            if i < m and scores[i] > thr:
                ls[pmin], li[pmin] = scores[i], i
                pmin = int(np.argmin(ls))                     # the first slot among equal minima
                thr = ls[pmin]
    order = np.lexsort((li, -ls))
    return li[order]


# ---------------------------------------------------------------------------------------------------------------------------
# The cases: one per form of the dispatch, the smallest catalogue that reaches the form, and both sides of every boundary
# where the form changes with the catalogue size.  r per case so that both conditions of test_eval_topk_restatement hold.
Case = namedtuple("Case", "m_items d K r frac_bits n_eval copies seed form")


def _c(m_items, d, K, form, r=4, frac_bits=0, n_eval=None, copies=1, seed=0):
    if n_eval is None:
        n_eval = 40 if m_items > 100000 else 150
    return Case(m_items, d, K, r, frac_bits, n_eval, copies, seed, form)


CASES = [
    _c(1000, 32, 7, "one part", n_eval=1),
    _c(4095, 64, 20, "one part", n_eval=127),
    _c(3000, 128, 50, "one part", n_eval=128),
    _c(3000, 256, 64, "one part", n_eval=129),
    _c(4095, 256, 20, "one part"),
    _c(3000, 32, 20, "one part"),
    _c(4096, 32, 20, "three parts, 16-bit ids"),
    _c(10007, 64, 20, "three parts, 16-bit ids", n_eval=160),
    _c(196416, 64, 20, "three parts, 16-bit ids: the last such size"),
    _c(196417, 64, 20, "two parts, int32 ids: the first size past it"),
    _c(10007, 64, 50, "two parts, 16-bit ids, K > 20"),
    _c(130944, 32, 64, "two parts, 16-bit ids, K > 20: the last such size"),
    _c(130945, 32, 64, "one part: the first size past it"),
    _c(10007, 128, 20, "d = 128: two parts, 16-bit ids, single tile buffer"),
    _c(10007, 128, 50, "d = 128, K > 20: one part"),
    _c(10007, 256, 20, "d = 256 at >= 4096 items: one part"),
    _c(10007, 256, 64, "d = 256 at >= 4096 items, 64-slot lists: one part"),
    # 10-bit values (the m plane carries bits); the ties come from item rows that are copies of each other, a third of the
    # catalogue apart: in different tiles and, split over parts, in different parts
    _c(3000, 32, 20, "one part, 10-bit values, copied rows", r=512, frac_bits=6, copies=3),
    _c(10008, 64, 20, "three parts, 10-bit values, copied rows", r=512, frac_bits=6, copies=3),
    _c(10008, 64, 50, "two parts, 10-bit values, copied rows", r=512, frac_bits=6, copies=3),
    # large K through lgcn_eval_topk_ex
    _c(300, 32, 256, "large K, one part"),
    _c(3001, 64, 65, "large K, one part"),
    _c(10007, 128, 128, "large K, parts"),
    _c(10007, 256, 256, "large K, parts"),
    _c(10008, 64, 100, "large K, parts, 10-bit values, copied rows", r=512, frac_bits=6, copies=3),
]


def case_id(c):
    return f"{c.m_items}x{c.d}-K{c.K}-r{c.r}" + (f"-n{c.n_eval}" if c.n_eval not in (40, 150) else "")


def train_lists(rng, n_users, m_items):
    """Train positives as the other evaluation tests build them: scattered ids, a cluster across a tile edge, ids around the
    boundaries of 2, 3 and 4 parts, the table's last two items for some users, none for others."""
    ntiles = (m_items + 31) // 32
    rows = []
    for u in range(n_users):
        c = set(rng.integers(0, m_items, rng.integers(0, 60)).tolist())
        t0 = int(rng.integers(0, max(1, ntiles - 1))) * 32
        c |= set(range(min(m_items, t0 + int(rng.integers(0, 8))), min(m_items, t0 + 32 + int(rng.integers(0, 20)))))
        for parts in (2, 3, 4):
            b = (ntiles * (u % parts) // parts) * 32
            c |= {min(m_items - 1, max(0, b - 1)), min(m_items - 1, b), min(m_items - 1, b + 1)}
        if u % 7 == 0:
            c |= {m_items - 1, max(0, m_items - 2)}
        if u % 11 == 0:
            c = set()
        rows.append(np.array(sorted(c), np.int32))
    return rows


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(1, np.int32)
    return ptr, idx


Problem = namedtuple("Problem", "E n_users users rows")


def make_problem(c):
    """Table, unsorted repeating user list and train lists of a case, from a seed that is the case."""
    rng = np.random.Generator(np.random.PCG64([c.m_items, c.d, c.K, c.r, c.seed]))
    n_users = 60 if c.m_items > 100000 else 300
    E = exact_table(n_users, c.m_items, c.d, c.r, c.frac_bits, rng)
    if c.copies > 1:
        blk = (c.m_items + c.copies - 1) // c.copies
        for q in range(1, c.copies):
            n = min(blk, c.m_items - q * blk)
            E[n_users + q * blk:n_users + q * blk + n] = E[n_users:n_users + n]
    users = rng.integers(0, n_users, c.n_eval).astype(np.int32)
    if c.n_eval > 4:
        users[-1] = users[0]                                  # a repeat, whatever the draw
    rows = train_lists(rng, n_users, c.m_items)
    return Problem(E, n_users, users, rows)


@lru_cache(maxsize=2)
def case_reference(c):
    p = make_problem(c)
    return p, rank_reference(p.E, p.n_users, p.users, p.rows, c.K)
