"""The evaluation problem that tests/test_gpu_eval_large_k.py and the `eval` kind of tools/ab_bitwise.py share: a Gaussian table, an
unsorted repeating user list and train positives placed where the item sweep changes path."""
import numpy as np


def problem(m_items, d, n_users=300, n_eval=257, seed=0):
    """Random table, train positives clustered across tile and part edges and at the table's end, an unsorted repeating user
    list."""
    rng = np.random.Generator(np.random.PCG64(seed + m_items + d))
    E = rng.standard_normal((n_users + m_items, d)).astype(np.float32)
    users = rng.integers(0, n_users, n_eval).astype(np.int32)
    ntiles = (m_items + 31) // 32
    rows = []
    for u in range(n_users):
        c = set(rng.integers(0, m_items, rng.integers(0, 60)).tolist())
        t0 = int(rng.integers(0, max(1, ntiles - 1))) * 32
        c |= set(range(t0 + int(rng.integers(0, 8)), min(m_items, t0 + 32 + int(rng.integers(0, 20)))))     # across a tile edge
        for parts in (2, 3, 4):
            b = (ntiles * (u % parts) // parts) * 32                                                    # around a part boundary
            c |= {min(m_items - 1, max(0, b - 1)), min(m_items - 1, b), min(m_items - 1, b + 1)}
        if u % 7 == 0:
            c |= {m_items - 1, m_items - 2}
        if u % 11 == 0:
            c = set()
        rows.append(np.array(sorted(c), np.int32))
    return E, users, rows


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(1, np.int32)
    return ptr, idx
