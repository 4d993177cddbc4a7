"""The slot-form losses in a context LARGER than the batch, and a smaller batch after a larger one, on the GPU (-m gpu): the
in-batch softmax (plain; cosine + logQ), the mixed pool (R_max = 16, steps at R = 1 and R = 5), DirectAU and the multi-negative
sampled softmax, on the graph and table of tests/storage_cases.py.

Why.  Every other test that judges these steps against float64 creates its context with max_batch = B, so the workspace capacity
equals the padded batch.  The workspaces are carved by the CAPACITY (InBatchWs / DirectAuWs in csrc/lgcn_ctx.h: `part` holds 2
cap parts(cap) floats, ib_invu() recomputes its offset from cap, the mixed carving holds (1 + R_max) cap item rows) while the
kernels index by the padded BATCH.  Training runs at capacity 2048 with a shorter last batch every epoch.  The "epoch equals the
loop of steps" tests do run B < cap, but with the same capacity and the same sequence on both sides: a wrong offset, or a read of
rows that the previous larger batch left behind, gives the same wrong bits twice.

1  capacity   one context of capacity 2048; from the same state the steps B = 1, 33, 260 and 705, each judged against float64 by
              the family's own _judge and bounds (tests/test_gpu_inbatch.py, test_gpu_inbatch_scores.py, test_gpu_inbatch_mix.py,
              test_gpu_directau.py, test_gpu_softmax.py: nothing new is derived here), and compared BIT FOR BIT -- per-sample terms,
              loss_out, table, both Adam moments -- with the same step in a context whose capacity is the batch (for the mixed pool:
              whose R_max is the step's R as well).  The arithmetic is indexed by B alone and the sums meet in fixed point or in a
              fixed order, so the capacity must not show in any bit.
2  sequence   in one context of capacity 2048 the steps B = 2048 -> 33 -> 705 -> 1 -> 2048, every one judged against float64 from
              the GPU's own state before it: the rows of the workspace that the larger batch left behind must not be read.
The mixed pool runs without logQ here: its logQ vector is a function of --bpr_batch and --neg_ratio (the mixture's expected
count), so two contexts of different capacity would be given different inputs.  Every test prints the shares its judge prints."""
import numpy as np
import pytest
import torch

import directau_restatement as DA
import inbatch_mix_bounds as MB
import inbatch_mix_restatement as IM
import inbatch_restatement as IB
import multineg_restatement as MN
import storage_cases as SC
import test_gpu_directau as TD
import test_gpu_inbatch as TI
import test_gpu_inbatch_mix as TM
import test_gpu_inbatch_scores as TS
import test_gpu_softmax as SMT
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 2048
CAPACITY_BS = (1, 33, 260, 705)
SEQUENCE_BS = (2048, 33, 705, 1, 2048)
R_MAX = 16
_dev = TI._dev

assert all(B < CAP for B in CAPACITY_BS) and IB.parts(CAP) == 8 and {IB.parts(B) for B in CAPACITY_BS} == {1, 2, 3}
assert SEQUENCE_BS[0] == CAP and all(b < a or b == CAP for a, b in zip(SEQUENCE_BS, SEQUENCE_BS[1:]) if a == CAP)


class _Family:
    """One loss: how its model is made at a capacity, its batch of B samples, the device call and the float64 judge."""
    d, K, mode, reg = 64, 2, "fp32", "propagated"

    def model(self, pkg, path, cap, R=None):
        return TI._model(pkg, path, self.mode, self.d, self.K, self.reg, dl=0, batch=cap, **self.cfg(R))

    def step(self, m, batch):
        return m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2] if len(batch) > 2 else np.zeros(len(batch[0]), np.int64)))

    def ratio(self, B):
        return None


class _InBatch(_Family):
    d, K, mode, reg, tau = 64, 1, "fp32", "propagated", 0.2

    def cfg(self, R):
        return dict(loss='inbatch', softmax_temp=self.tau)

    def batch(self, B, seed):
        return IB.make_batch(B, seed)

    def judge(self, pkg, ds, m, batch, step_no, tag):
        return TI._judge(pkg, m, batch, self.K, self.d, self.mode, self.reg, TI._tau32(self.tau), step_no, tag)[0]


class _InBatchCosineLogq(_InBatch):
    d, K, mode, reg, tau = 128, 2, "bf16", "ego", 0.1

    def cfg(self, R):
        return TS._cfg(self.tau, "cosine", True)

    def judge(self, pkg, ds, m, batch, step_no, tag):
        return TS._judge(pkg, ds, m, batch, self.K, self.d, self.mode, self.reg, TI._tau32(self.tau), step_no, tag, "cosine", True)[0]


class _Mix(_Family):
    d, K, mode, reg, tau, score = 32, 2, "fp32", "ego", 0.2, "cosine"

    def __init__(self, ratios):
        self.ratios = ratios                                                # B -> the step's R

    def ratio(self, B):
        return self.ratios[B]

    def cfg(self, R):
        return TM._cfg(self.tau, R_MAX if R is None else R, self.score, False)

    def batch(self, B, seed):
        return IM.make_batch(B, self.ratios[B], seed)

    def judge(self, pkg, ds, m, batch, step_no, tag):
        return TM._judge(pkg, ds, m, batch, self.K, self.d, self.mode, self.reg, MB.tau32(self.tau), step_no, tag, self.score, False)[0]


class _MixDot(_Mix):
    d, K, mode, reg, tau, score = 256, 1, "bf16", "propagated", 0.1, "dot"


class _DirectAu(_Family):
    d, K, mode, reg, gamma = 64, 1, "fp32", "ego", 1.0

    def cfg(self, R):
        return TD._cfg(self.gamma)

    def batch(self, B, seed):
        return DA.make_batch(B, seed)

    def judge(self, pkg, ds, m, batch, step_no, tag):
        return TD._judge(pkg, m, batch, self.K, self.d, self.mode, self.reg, self.gamma, step_no, tag)[0]


class _Softmax(_Family):
    d, K, mode, reg, tau, R = 64, 3, "bf16", "propagated", 0.2, 5

    def model(self, pkg, path, cap, R=None):
        return SMT._model(pkg, path, self.mode, self.d, self.K, self.reg, dl=0, batch=cap, loss='softmax', softmax_temp=self.tau, neg_ratio=self.R)

    def batch(self, B, seed):
        return MN.make_batches(self.d, self.K, self.R, seed, sizes=(B,))[0]

    def judge(self, pkg, ds, m, batch, step_no, tag):
        return SMT._judge(pkg, m, batch, self.R, self.K, self.d, self.mode, self.reg, SMT._tau32(self.tau), step_no, tag)[0]


# the mixed pool steps at R = 1 and R = 5 in a context of R_max = 16; (2048, 5) is left out of the sequence: its float64
# restatement holds a dozen [2048, 12288] arrays
FAMILIES = {
    "inbatch": _InBatch(),
    "inbatch-cosine-logq": _InBatchCosineLogq(),
    "mix-cosine": _Mix({1: 5, 33: 1, 260: 5, 705: 1, 2048: 1}),
    "mix-dot": _MixDot({1: 1, 33: 5, 260: 1, 705: 5, 2048: 1}),
    "directau": _DirectAu(),
    "softmax": _Softmax(),
}
assert {F.ratios[B] for F in FAMILIES.values() if isinstance(F, _Mix) for B in CAPACITY_BS} == {1, 5}
assert all({F.ratios[B] for F in FAMILIES.values() if isinstance(F, _Mix)} == {1, 5} for B in CAPACITY_BS)


def _snapshot(m):
    st = m._dev
    return m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone()


def _restore(m, snap):
    with torch.no_grad():
        m._table.copy_(snap[0]); m._dev['adam_m'].copy_(snap[1]); m._dev['adam_v'].copy_(snap[2])
    m.set_adam_step(0)
    m.invalidate_cache()


def _bits(m, out, B):
    return dict(loss_out=out.detach().clone(), terms=m._dev['terms'][:2 * B].clone(), table=m._table.detach().clone(),
                M=m._dev['adam_m'].clone(), V=m._dev['adam_v'].clone())


def _differing(a, b):
    """The names of the tensors of two _bits that differ in any bit (fp32 as int32: -0 is not 0, a NaN equals itself)."""
    return [k for k in a if not torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32))]


# ---- 1. a context larger than the batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_a_step_in_a_larger_context(pkg, storage_graph, fam):
    """Capacity 2048, B = 1, 33, 260, 705 from the same state: within the family's float64 bounds, and bit for bit the step of a
    context whose capacity is B."""
    F = FAMILIES[fam]
    try:
        ds, big = F.model(pkg, storage_graph, CAP)
        st = big._state(max_batch=CAP, need_ctx=True)
        assert st['max_batch'] == CAP
        start = _snapshot(big)
        bad, got = [], {}
        for B in CAPACITY_BS:
            batch = F.batch(B, seed=3)
            tag = f"{fam} B={B} in capacity {CAP}" + (f" R={F.ratio(B)} of {R_MAX}" if F.ratio(B) else "")
            share = F.judge(pkg, ds, big, batch, 1, tag)
            big.check_device_errors()
            assert big._dev['max_batch'] == CAP and not bool(big._dev['G64'].any())      # (the context was not remade)
            bad += [(tag, k, v) for k, v in share.items() if not v <= 1.0]
            _restore(big, start)
            got[B] = _bits(big, F.step(big, batch), B)                    # the same step again, for its bits
            big.check_device_errors()
            _restore(big, start)
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
        diff = []
        for B in CAPACITY_BS:
            ds2, small = F.model(pkg, storage_graph, B, R=F.ratio(B))
            s2 = small._state(max_batch=B, need_ctx=True)
            assert s2['max_batch'] == B and all(torch.equal(a, b) for a, b in zip(_snapshot(small), start))
            want = _bits(small, F.step(small, F.batch(B, seed=3)), B)
            small.check_device_errors()
            assert float((want["table"] - start[0]).abs().max()) > 0.0      # (it stepped)
            diff += [(B, k) for k in _differing(got[B], want)]
        assert not diff, ("capacity 2048 against capacity B: not the same bits (B, tensor)", diff)
    finally:
        pkg.world.configure([])


# ---- 2. a smaller batch after a larger one -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_smaller_batches_after_larger_ones(pkg, storage_graph, fam):
    """One context of capacity 2048, B = 2048 -> 33 -> 705 -> 1 -> 2048: every step within the family's float64 bounds from the
    GPU's own state before it."""
    F = FAMILIES[fam]
    try:
        ds, m = F.model(pkg, storage_graph, CAP)
        assert m._state(max_batch=CAP, need_ctx=True)['max_batch'] == CAP
        bad = []
        for i, B in enumerate(SEQUENCE_BS):
            tag = f"{fam} sequence step {i + 1} B={B}" + (f" R={F.ratio(B)} of {R_MAX}" if F.ratio(B) else "")
            share = F.judge(pkg, ds, m, F.batch(B, seed=10 + i), i + 1, tag)
            m.check_device_errors()
            assert m._dev['max_batch'] == CAP and m.adam_step == i + 1 and not bool(m._dev['G64'].any())
            bad += [(tag, k, v) for k, v in share.items() if not v <= 1.0]
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])
