"""The contract of lgcn_eval_pop_metrics (include/lgcn_hip.h), restated in numpy from the definitions: int64 /
float64, np.isin for the hits, np.sort for the Gini numerator in its sorted-rank form, a Python loop over the slots.  It shares
nothing with the kernels' formulation (no ballots, no buckets, no histogram) and is what the host and GPU tests compare with.

Inputs: topk [n, K] ranked ids (ids of a list distinct; an id outside [0, m) counts nowhere), the test CSR over the slots
(test_ptr [n + 1], test_items ascending per slot), pop [m] train interactions, groups [m] group ids (an id >= G is in no
reported group), ks the cut-offs."""
import numpy as np


def gini_numerator(e):
    """sum_{i<j} |e_i - e_j| as a Python int: sum_i (2 rank_i - m - 1) e_(i) over the ascending sort (ranks 1-based)."""
    e = np.sort(np.asarray(e, np.int64))
    m = len(e)
    return int(np.sum((2 * np.arange(1, m + 1, dtype=np.int64) - m - 1) * e))


def gini_numerator_pairs(e):
    """The definition itself, O(m^2): for small cases."""
    e = np.asarray(e, np.int64)
    return int(np.abs(e[:, None] - e[None, :]).sum() // 2)


def restate(topk, test_ptr, test_items, pop, groups, G, ks):
    topk = np.asarray(topk, np.int64)
    test_ptr = np.asarray(test_ptr, np.int64)
    test_items = np.asarray(test_items, np.int64)
    pop = np.asarray(pop, np.int64)
    groups = np.asarray(groups, np.int64)
    n, m, nk = topk.shape[0], len(pop), len(ks)
    per_slot = np.zeros((n, nk, 2, G), np.float64)
    list_counts = np.zeros((nk, G), np.int64)
    valid = np.zeros(nk, np.int64)
    pop_sum = np.zeros(nk, np.int64)
    exposure = np.zeros((nk, m), np.int64)
    group_slots = np.zeros(G, np.int64)
    for s in range(n):
        T = test_items[test_ptr[s]:test_ptr[s + 1]]
        Tg = groups[T[(T >= 0) & (T < m)]]
        t = np.array([(Tg == g).sum() for g in range(G)], np.int64)
        group_slots += t > 0
        for q, k in enumerate(ks):
            L = topk[s, :k]
            L = L[(L >= 0) & (L < m)]
            hit = np.isin(L, T)
            valid[q] += len(L)
            pop_sum[q] += pop[L].sum()
            exposure[q, np.unique(L)] += 1
            for g in range(G):
                in_g = groups[L] == g
                h = int((hit & in_g).sum())
                list_counts[q, g] += int(in_g.sum())
                per_slot[s, q, 0, g] = h / len(T) if len(T) else 0.0
                per_slot[s, q, 1, g] = h / int(t[g]) if t[g] else 0.0
    sums = per_slot.sum(axis=0)
    covered = (exposure > 0).sum(axis=1).astype(np.int64)
    sum_e = exposure.sum(axis=1)
    gini_num = np.array([gini_numerator(exposure[q]) for q in range(nk)], np.int64)
    counts = np.concatenate([list_counts, valid[:, None], pop_sum[:, None], covered[:, None], sum_e[:, None], gini_num[:, None]], axis=1)
    ng = group_slots.astype(np.float64)
    out = {'per_slot': per_slot, 'sums': sums, 'counts': counts, 'group_slots': group_slots, 'exposure': exposure,
           'recall_share': sums[:, 0, :].T / max(n, 1),
           'recall_by_group': np.array([[sums[q, 1, g] / ng[g] if ng[g] else 0.0 for q in range(nk)] for g in range(G)]).reshape(G, nk),
           'list_share': np.array([[list_counts[q, g] / valid[q] if valid[q] else 0.0 for q in range(nk)] for g in range(G)]).reshape(G, nk),
           'arp': np.array([pop_sum[q] / valid[q] if valid[q] else 0.0 for q in range(nk)]),
           'coverage': covered / float(m),
           'gini': np.array([int(gini_num[q]) / (m * int(sum_e[q])) if sum_e[q] else 0.0 for q in range(nk)]),
           'group_users': group_slots.copy()}
    return out
