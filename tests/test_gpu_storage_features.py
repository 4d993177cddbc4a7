"""The fused step with layer weights (--layer_weights) and with edge dropout (--dropout 1 --keepprob p), launch by launch against
float64 (-m gpu), at every embedding width (32 / 64 / 128 / 256: the four lane geometries) and both storage types (fp32, bf16) the
two features are built for -- the instantiations k_spmm<.., MODE | M_WTS> of launch_spmm_wts, k_triplet<.., WTS>,
k_triplet_dense<.., WTS>, k_spmm<.., DROP> of launch_spmm_d in all five modes and k_triplet<.., DROP>.  The machinery is
tests/test_gpu_storage_step.py's (chain of custody: every link restated in float64 on the numbers the GPU itself stored); the
cases are storage_cases.FEATURE_CASES / FEATURE_K4_CASES / FEATURE_EPOCH_CASES on the same graph, table rows and batches; the
restatement's two axes are pinned to float64 torch autograd by tests/test_storage_restatement.py on the CPU.

What a feature changes in the judgement:
  forward tables   dropout: Graph.spmm_drop(x, keep, seed, step = the step counter, y_dtype = the storage type) for every forward
                   layer, asserted torch.equal to st['act'][k] wherever the step leaves the table intact; weights: the default's.
  restatement      S.step(.., weights = w, A_fwd = A_drop, A_bwd = A_drop^T): slot rows e = sum_k w[k] X_k without a division, G
                   unscaled, backward launch k: w[k-1] G + w_in (A h); under dropout the forward links and the slot rows' last
                   layer on A_drop, the backward chain on its explicit transpose (the mask is not symmetric: the CPU test shows
                   that A_bwd = A_fwd misses the gradient by a quarter of its size).
  mask             per step, the mask exported on the model's own graph for the step counter equals the host restatement
                   (_keep_host) and keeps keep +- 0.05 of the entries; A_drop is built from the restatement.
  outside rows     rows outside the reach of the DROPPED graph's transpose are exactly zero in every stored backward table and
                   zero to the recovery slack in the gradient: a backward launch on the untransposed or undropped graph, or with
                   another step's mask, writes there.
  fp32 storage     stored tables are compared with the fp32 bound alone (no half-ulp term).
BOUNDS: storage_cases' module docstring, "THE TWO FEATURES": the weighted slot row (K + 2) u T_w + |w[K]| delta_last with T_w =
sum_k |w[k]| |X_k|; delta_Gs = delta_G + u |G| (gdiv = 1: one rounding); the weighted backward |w_add| delta_Gs + u |w_add G| +
|w_in| (|A| delta_Gs + SpMM bound) + u |w_in| |A| |h| + u (|w_add G| + |w_in| |A| |h|), nothing for a zero weight; dropout: every
SpMM bound on |A_drop| / |A_drop^T| (the staged weight fl32(val fl32(1 / keep)) is the restatement's own number); bf16:
stored_bound as it is; K = 4: (K - 1) 2^-8 sum_j |w[j]| |B|^j |G| on the backward's matrix B.  Nothing is fitted to what the GPU
returns.  Every test prints the largest share of each bound it used (profiles/storage_step/README.md)."""
import pytest

import storage_cases as SC
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_storage_step import _epoch_vs_steps, _run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SC.FEATURE_CASES, ids=SC.case_id)
def test_feature_step_launch_by_launch(pkg, storage_graph, case):
    """Every link of four steps (64 / 64 / 37 / 1 triplets) with layer weights or dropout on the GPU's own stored numbers: the d x
    storage x K x dense_last grid of each feature, the zero-weight sets, the hub plan, reg_rows = ego and keep 0.9."""
    _run_case(pkg, storage_graph, case)


@pytest.mark.parametrize("case", SC.FEATURE_K4_CASES, ids=SC.case_id)
def test_feature_four_layers_end_to_end(pkg, storage_graph, case):
    """K = 4 (bf16, d = 128): the recovered gradient against the float64 chain without backward storage on the GPU's own forward
    tables, within storage_cases.feature_k4_allowance + the chained fp32 bounds (test_four_layers_end_to_end)."""
    _run_case(pkg, storage_graph, case, end_to_end=True)


@pytest.mark.parametrize("case", SC.FEATURE_EPOCH_CASES, ids=SC.case_id)
def test_feature_epoch_equals_single_steps_bitwise(pkg, storage_graph, case):
    """lgcn_train_epoch against the loop of single steps with a feature on (bf16, d 32 / 128, K 2 / 3, both last layers): losses,
    table and both Adam moments bit for bit over six steps.  The only observer of the Adam epilogue's bf16 shadow rows in the
    M_WTS and DROP instantiations; for dropout it also shows the mask following the step counter inside the C loop."""
    _epoch_vs_steps(pkg, storage_graph, case)
