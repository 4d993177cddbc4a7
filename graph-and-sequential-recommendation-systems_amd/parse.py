"""Flag surface of the reference's parse.py (parse.py:16-114): the same 34 flags
with the same names, types and defaults, plus additive flags (marked NEW) whose
defaults reproduce the reference's behaviour."""
import argparse


def build_parser():
    p = argparse.ArgumentParser(description="Go LightGCN")
    # core training parameters                                    parse.py:20-37
    p.add_argument('--bpr_batch', type=int, default=2048)
    p.add_argument('--recdim', type=int, default=64)
    p.add_argument('--layer', type=int, default=3)
    p.add_argument('--lr', type=float, default=0.001)
    p.add_argument('--decay', type=float, default=1e-4)
    p.add_argument('--dropout', type=int, default=0)
    p.add_argument('--keepprob', type=float, default=0.6)
    p.add_argument('--epochs', type=int, default=1000)
    p.add_argument('--testbatch', type=int, default=100)
    # dataset & paths                                              parse.py:40-45
    p.add_argument('--dataset', type=str, default='gowalla')
    p.add_argument('--checkpoint_dir', type=str, default='./checkpoints')
    p.add_argument('--topks', type=str, default='[20]')
    # logging & reproducibility                                    parse.py:48-61
    p.add_argument('--tensorboard', type=int, default=1)
    p.add_argument('--comment', type=str, default='lgn')
    p.add_argument('--load', type=int, default=0)
    p.add_argument('--pretrain', type=int, default=0)
    p.add_argument('--seed', type=int, default=2020)
    p.add_argument('--model', type=str, default='lgn')
    p.add_argument('--a_fold', type=int, default=100)
    p.add_argument('--A_split', dest='A_split', action='store_true')
    p.add_argument('--no-A_split', dest='A_split', action='store_false')
    p.set_defaults(A_split=False)
    # global smoothing / PPR                                       parse.py:69-74
    p.add_argument('--exp_smooth_beta', type=float, default=0.5)
    p.add_argument('--use_ppr_weights', action='store_true')
    p.add_argument('--ppr_weights_path', type=str, default=None)
    # scheduler                                                    parse.py:77-82
    p.add_argument('--use_scheduler', action='store_true')
    p.add_argument('--sched_milestones', type=str, default='[120,240,360,480]')
    p.add_argument('--sched_gamma', type=float, default=0.5)
    # popularity gate                                              parse.py:85-94
    p.add_argument('--use_pop_gate', action='store_true')
    p.add_argument('--pop_hidden', type=int, default=32)
    p.add_argument('--gate_hidden', type=int, default=64)
    p.add_argument('--gate_entropy_coeff', type=float, default=1e-4)
    p.add_argument('--pop_gate_temp', type=float, default=1.0)
    # item-item adjacency                                          parse.py:97-102
    p.add_argument('--use_item_item', action='store_true')
    p.add_argument('--i2i_path', type=str, default=None)
    p.add_argument('--i2i_alpha', type=float, default=0.0)
    # miscellaneous                                                parse.py:105-112
    p.add_argument('--multicore', type=int, default=0)
    p.add_argument('--resume', action='store_true')
    p.add_argument('--resume_path', type=str, default=None)
    p.add_argument('--save_every', type=int, default=10)
    # ---- NEW (additive) ----------------------------------------------------
    p.add_argument('--sampler', type=str, default='auto', choices=['auto', 'cpp', 'python'],
                   help="NEW: 'cpp' = sampling.cpp stream, 'python' = numpy fallback stream, "
                        "'auto' = cpp unless a user has no positives")
    p.add_argument('--act_dtype', type=str, default='fp32', choices=['fp32', 'bf16', 'fp8'],
                   help='NEW: storage type of propagated layer activations, forward and backward (accumulation, parameters and Adam '
                        'state stay fp32). fp8 = OCP E4M3 with a power-of-two fp32 scale per row; d >= 64, default model only')
    p.add_argument('--xcd_remap', type=int, default=1,
                   help='NEW: give every XCD a contiguous range of graph rows')
    p.add_argument('--row_order', type=str, default='xcd', choices=['natural', 'rcm', 'cocluster', 'xcd'],
                   help='NEW: processing order of graph rows in the SpMM kernels (L2 locality; results unchanged)')
    p.add_argument('--prefetch_epoch', type=int, default=1,
                   help='NEW: 1 (default) = sample/shuffle/upload epoch e+1 while epoch e runs on the GPU (same triplets: the '
                        'sampler and shuffle streams do not depend on training; Gowalla epoch 72.5 -> 61 ms); 0 = at the start '
                        'of each epoch, for code that draws from those RNG streams between epochs')
    p.add_argument('--dense_last', type=str, default='auto', choices=['auto', '0', '1'],
                   help='NEW: last forward layer on the batch rows only (0), densely (1), or whichever is cheaper for '
                        'this graph and batch size (auto)')
    p.add_argument('--fused_variants', type=int, default=1,
                   help='NEW: 1 = --use_pop_gate / --use_item_item train inside the fused HIP step; 0 = autograd path (torch MLPs '
                        'and torch Adam around the HIP propagation kernels)')
    p.add_argument('--hub_nnz', type=int, default=0,
                   help='NEW: graph rows with more non-zeros than this get their last-layer row from a whole-chip SpMM once per '
                        'step instead of from every triplet that names them (0 = library default 131072, < 0 = off)')
    p.add_argument('--gpu_sampler', type=int, default=1,
                   help='NEW: 1 = the cpp-mode BPR sampler runs on the GPU at every --neg_ratio (same rand() stream, same rows of '
                        '2 + neg_ratio ids); 0 = on the host')
    p.add_argument('--lazy_loss', type=int, default=0,
                   help='NEW: 1 = BPRLoss.stageOne returns a float-like DeferredLoss that is read from the device only when looked at '
                        '(the reference returns loss.cpu().item(): a host round trip per step); 0 = a Python float, as the reference')
    p.add_argument('--gpu_shuffle', type=int, default=1,
                   help='NEW: 1 = the epoch permutation (numpy legacy shuffle: MT19937 + Fisher-Yates, same stream, same permutation) is '
                        'computed on the GPU; 0 = on the host')
    p.add_argument('--eval_fused', type=int, default=1,
                   help='NEW: 1 = Procedure.Test through the fused HIP kernels (MFMA scores + mask + top-k, metrics on device); '
                        '0 = torch matmul/topk harness')
    p.add_argument('--rank_metrics', type=int, default=0,
                   help='NEW: 1 = Procedure.Test ranks through lgcn_eval_ranks / lgcn_eval_rank_metrics: the position of every test item '
                        'in the full ranking from one item sweep, so any cut-off up to the catalogue size stays on the GPU, and the '
                        "result also holds 'auc' (utils.AUC) and 'mrr'; 0 (default) = Test as before")
    p.add_argument('--pop_metrics', type=int, default=0, choices=[0, 1],
                   help='NEW: 1 = Procedure.Test also reports, at every cut-off of --topks and from the lists the fused evaluation ranked '
                        '(lgcn_eval_pop_metrics, on the GPU): recall split by item-popularity group (recall_share, recall_by_group), the '
                        'share of every group in the lists (list_share), the average popularity of the recommended items (arp), catalogue '
                        'coverage and the Gini index of item exposure; 0 (default) = Test as before. Not with --rank_metrics 1 or '
                        '--eval_fused 0')
    p.add_argument('--pop_groups', type=str, default="[0.2]",
                   help='NEW: boundaries of the popularity groups of --pop_metrics: a strictly increasing list of at most 7 values in '
                        '(0, 1), cumulative shares of the items ranked by train popularity (group 0 = the most popular). [0.2] = the '
                        '20 %% head and the 80 %% tail')
    p.add_argument('--pop_group_by', type=str, default='items', choices=['items', 'interactions'],
                   help="NEW: what the shares of --pop_groups are taken of: 'items' (default) or the train 'interactions'")
    p.add_argument('--reg_rows', type=str, default='propagated', choices=['propagated', 'ego'],
                   help="NEW: rows the L2 term of bpr_loss is taken on. 'propagated' (default) = this reference (model.py:173: the "
                        "propagated rows of the batch); 'ego' = upstream LightGCN (userEmb0 / posEmb0 / negEmb0, the embedding "
                        "tables' own rows) -- the loss behind the recorded 1000-epoch run and the README table the reference keeps")
    p.add_argument('--i2i_build', type=str, default='none', choices=['none', 'cooc', 'jaccard', 'pmi'],
                   help='NEW: with --use_item_item and no --i2i_path, build the item-item graph from the train baskets on the GPU '
                        '(preprocess_instacart_i2i.build_item_item with this weighting); none (default) = as the reference: no '
                        'file, no item-item branch. One basket per user with train items, in user order: the graph of the module\'s '
                        'CLI (one basket per line of train.txt) whenever every user is one line')
    p.add_argument('--i2i_topk', type=int, default=50, help='NEW: neighbours kept per item by --i2i_build (1..256)')
    p.add_argument('--i2i_min_basket', type=int, default=1, help='NEW: --i2i_build skips baskets with fewer items')
    p.add_argument('--layer_weights', type=str, default='mean',
                   help="NEW: weights of the layer combination out = sum_k w_k X_k, in the fused step, the autograd path and evaluation. "
                        "'mean' (default) = the reference: 1/(K+1) each; 'exp' = w_k ~ beta^k with --exp_smooth_beta, normalised; "
                        "'ppr' = w_k ~ alpha (1-alpha)^k with --ppr_alpha, normalised (--use_ppr_weights means this); or a literal list "
                        "of K+1 floats such as \"[0.4,0.3,0.2,0.1]\", taken as written. fp32 / bf16 storage, single GPU, default model")
    p.add_argument('--ppr_alpha', type=float, default=0.15,
                   help="NEW: teleport probability of --layer_weights ppr (the default of the reference's compute_ppr.py)")
    p.add_argument('--neg_ratio', type=int, default=1,
                   help='NEW: negatives drawn per sampled positive (1..16). 1 (default) = the reference: triplets. R > 1 trains on '
                        'samples (u, p, n_1..n_R) in the fused step -- the loss of the flattened B*R triplets, with the user and '
                        'positive rows read and added once per sample. Native host sampler (--sampler cpp), fp32 / bf16 storage, '
                        'single GPU, default model, dense last layer')
    p.add_argument('--loss', type=str, default='bpr', choices=['bpr', 'softmax', 'inbatch', 'directau'],
                   help='NEW: loss of the fused step. bpr (default) = the reference: -mean logsigmoid(x) over the (flattened) triplets. '
                        'softmax = the sampled-softmax loss: the positive competes against all --neg_ratio negatives of its sample in '
                        'one log-sum-exp at --softmax_temp, log(1 + sum_r exp(-x_r / tau)), one term per sample; the "bpr" slot of the '
                        'reported loss then holds it. inbatch = the in-batch sampled softmax: every user of the batch scores against every '
                        'positive of the batch at --softmax_temp and the other samples\' positives are the negatives (the same item, and '
                        'other positives of the same user, are left out); the sampled negatives are not used, so --neg_ratio must be 1. '
                        'directau = alignment and uniformity (DirectAU), no negatives at all: mean |x - y|^2 over the samples plus --au_gamma '
                        'times the mean over users and items of log mean_{b<c} exp(-2 |x_b - x_c|^2), x and y the rows over their norms; '
                        'the "bpr" slot of the reported loss then holds it, the sampled negatives are not used (--neg_ratio 1) and '
                        'evaluation still ranks by the inner product. fp32 / bf16 storage, single GPU, default model, dense last layer')
    p.add_argument('--au_gamma', type=float, default=1.0,
                   help='NEW: weight gamma >= 0 of the uniformity term of --loss directau (0 = the alignment term alone)')
    p.add_argument('--softmax_temp', type=float, default=1.0,
                   help='NEW: temperature tau > 0 of --loss softmax (at --neg_ratio 1 and tau = 1 the loss is the BPR loss) and of --loss inbatch')
    p.add_argument('--score', type=str, default='dot', choices=['dot', 'cosine'],
                   help='NEW: how --loss inbatch forms its scores. dot (default) = the inner product of the output rows. cosine = the inner '
                        'product of the rows over their norms, trained through the normalisation; evaluation then ranks by cosine too. The '
                        'scores lie in [-1, 1], so cosine wants --softmax_temp well below 1 (0.1 .. 0.2). --loss inbatch only')
    p.add_argument('--inbatch_logq', type=int, default=0, choices=[0, 1],
                   help='NEW: 1 = subtract log Q(item) = log(train degree) from every in-batch logit (the logQ correction: in-batch '
                        'negatives arrive in proportion to item popularity). 0 (default) = no correction. --loss inbatch only')
    p.add_argument('--inbatch_mix', type=int, default=0, choices=[0, 1],
                   help='NEW: 1 = mixed negative sampling for --loss inbatch: the --neg_ratio sampled negatives of all samples of the batch '
                        'are a pool shared by the whole batch, extra columns of every sample\'s score row in the same log-sum-exp '
                        '(--neg_ratio 1..16 is then legal); with --inbatch_logq 1 the correction is the log of the mixture, '
                        'log((B - 1) deg / sum deg + B R / m_items) with B = --bpr_batch. 0 (default) = in-batch negatives only. '
                        '--loss inbatch only')
    p.add_argument('--hard_neg', type=int, default=0,
                   help='NEW: M > 0 = dynamic negative sampling, DNS(M, N): the fused step scores the --neg_ratio R candidates of a sample '
                        'with the current model and trains the plain BPR triplet (u, p, n) on ONE of them -- a uniform pick among the M '
                        'hardest, keyed by --seed, the step counter and the sample (M = 1: the hardest; M = R: a uniform candidate). '
                        'Three gradient rows per sample instead of 2 + R. Needs --neg_ratio >= 2, M <= R and --loss bpr. 0 (default) = off. '
                        'fp32 / bf16 storage, single GPU, default model, dense last layer')
    p.add_argument('--data_path', type=str, default=None,
                   help='NEW: directory that holds <dataset>/train.txt (default: <root>/data)')
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)
