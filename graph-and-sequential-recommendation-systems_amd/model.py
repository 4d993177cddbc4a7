"""LightGCN, mirror of the reference's model.py (model.py:37-231) for the hot path.

Same constructor `(config, dataset)`, same parameters (`embedding_user.weight`
[n_users,d], `embedding_item.weight` [m_items,d] -> same state_dict keys), same
methods (`computer`, `getEmbedding`, `bpr_loss`, `getUsersRating`, `forward`) plus
the optional `invalidate_cache()` hook main.py:190-191 probes for.

All propagation / loss / optimiser arithmetic runs in the hand-written gfx950
kernels behind include/lgcn_hip.h.  There is no torch.sparse.mm path and no CPU
fallback: on a machine without a HIP device every compute method raises.

The fork's optional branches (8f-4) are supported on the autograd path: the
popularity gate (model.py:66-96,139-157,176-181: two small dense MLPs, torch ops) and the item-item
smoothing (model.py:99-109,228-229: one more CSR SpMM, the same HIP kernel on the item-item graph, with
its transpose in backward).  With either switched on, BPRLoss.stageOne is the reference's own sequence
(bpr_loss -> backward -> torch.optim.Adam over ALL parameters) with every propagation in the HIP
kernels; the fused single-launch-chain step covers the default model only.
"""
import ctypes as C

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from . import world
from . import _lib


def _act_code(name):
    return {'fp32': _lib.F32, 'bf16': _lib.BF16, 'fp8': _lib.FP8}[name]


def _act_tables(n_tables, N, d, act_dtype, dev):
    """workspace of n_tables [N,d] tables of a storage type, as one tensor whose leading index is the table (fp8 tables
    are byte blobs: rows + row scales, lgcn_table_bytes each)"""
    if act_dtype == _lib.FP8:
        return torch.zeros(n_tables, int(_lib.load().lgcn_table_bytes(N, d, _lib.FP8)), dtype=torch.uint8, device=dev)
    return torch.zeros(n_tables, N, d, dtype=torch.float32 if act_dtype == _lib.F32 else torch.bfloat16, device=dev)


def _check_layer_weights(w, K, what):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size != K + 1:
        raise ValueError(f"{what}: {w.size} layer weights for --layer {K} (K + 1 = {K + 1} are needed)")
    with np.errstate(over='ignore'):           # (an overflow becomes inf and is refused below)
        w32 = w.astype(np.float32)
    if not np.all(np.isfinite(w32)):
        raise ValueError(f"{what}: layer weights must be finite, got {w.tolist()}")
    if not np.any(w32 != 0):
        raise ValueError(f"{what}: layer weights are all zero")
    return w32


def load_ppr_weights(path, K, degrees=None):
    """--ppr_weights_path: a .npy of shape [K+1], or [N, K+1] as the reference's compute_ppr.py writes it.  That script's
    transition matrix is row-stochastic, so every node with a neighbour gets the same row alpha (1-alpha)^k / sum: that row
    is used.  Rows that differ by more than 1e-6 (fp32 file precision) mean per-node weights, which are not implemented.
    Rows of isolated nodes (degrees[i] == 0; [1, 0, ...] in the reference's output) are ignored -- the one deviation: they
    would only scale E0 rows that nothing propagates and no training triplet names."""
    w = np.load(path)
    if w.ndim == 1:
        return _check_layer_weights(w, K, f"--ppr_weights_path {path}")
    if w.ndim != 2 or w.shape[1] != K + 1:
        raise ValueError(f"--ppr_weights_path {path}: shape {w.shape} is neither [K+1] nor [N, K+1] for --layer {K}")
    if degrees is not None:
        degrees = np.asarray(degrees)
        if degrees.shape[0] != w.shape[0]:
            raise ValueError(f"--ppr_weights_path {path}: {w.shape[0]} rows for a graph of {degrees.shape[0]} nodes")
        w = w[degrees > 0]
    if w.shape[0] == 0:
        raise ValueError(f"--ppr_weights_path {path}: no row of a node with a neighbour")
    if float(np.abs(w.astype(np.float64) - w[0].astype(np.float64)).max()) > 1e-6:
        raise ValueError(f"--ppr_weights_path {path}: the rows of connected nodes differ: per-node weights are not implemented "
                         "(one weight vector for all nodes is)")
    return _check_layer_weights(w[0], K, f"--ppr_weights_path {path}")


def resolve_loss(config):
    """--loss bpr | softmax | inbatch | directau and --softmax_temp -> ('bpr' | 'softmax' | 'inbatch' | 'directau', temperature).
    ValueError: an unknown loss, or a temperature that is not a finite value > 0 (--loss directau has none: it is not looked at)."""
    kind = str(config.get('loss', 'bpr')).strip().lower()
    if kind not in ('bpr', 'softmax', 'inbatch', 'directau'):
        raise ValueError(f"--loss must be bpr, softmax, inbatch or directau, got {config.get('loss')!r}")
    tau = float(config.get('softmax_temp', 1.0))
    if kind == 'directau':
        return kind, 1.0
    if kind != 'bpr' and not (np.isfinite(tau) and tau > 0.0):
        raise ValueError(f"--loss {kind}: --softmax_temp must be a finite value > 0, got {tau}")
    return kind, tau


def resolve_au_gamma(config, loss_kind):
    """--au_gamma -> the weight of the uniformity term of --loss directau.  ValueError naming the flag: not a finite
    value >= 0.  Under any other loss the flag is not looked at."""
    if loss_kind != 'directau':
        return 1.0
    gamma = float(config.get('au_gamma', 1.0))
    if not (np.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"--loss directau: --au_gamma must be a finite value >= 0, got {gamma}")
    return gamma


def _unit_rows(x):
    """x [n, d] -> its rows over their norms; a row of norm 0 stays 0 (the inv(e) of DESIGN 4.20)."""
    n = x.norm(dim=1, keepdim=True)
    return x * torch.where(n > 0, 1.0 / n, torch.zeros_like(n))


def resolve_inbatch_scores(config, loss_kind):
    """--score dot | cosine and --inbatch_logq 0 | 1 -> ('dot' | 'cosine', bool).  Both are options of --loss inbatch:
    LgcnError naming the flag under any other loss; ValueError for a value that is neither."""
    score = str(config.get('score', 'dot')).strip().lower()
    if score not in ('dot', 'cosine'):
        raise ValueError(f"--score must be dot or cosine, got {config.get('score')!r}")
    lq = str(config.get('inbatch_logq', 0)).strip().lower()
    if lq not in ('0', '1', 'false', 'true'):
        raise ValueError(f"--inbatch_logq must be 0 or 1, got {config.get('inbatch_logq')!r}")
    lq = lq in ('1', 'true')
    if loss_kind != 'inbatch':
        if score == 'cosine':
            raise _lib.LgcnError(f"--score cosine is implemented for --loss inbatch only, not for --loss {loss_kind} "
                                 "(cosine scores for the sampled softmax are not implemented)")
        if lq:
            raise _lib.LgcnError(f"--inbatch_logq 1 is implemented for --loss inbatch only, not for --loss {loss_kind} "
                                 "(the correction is for negatives that arrive in proportion to item popularity)")
    return score, lq


def item_logq(items_D):
    """The logQ vector of --inbatch_logq 1: log of the train degree (zeros already 1 in the loader) in float64, rounded once to
    fp32.  The -log E that would make it a log-probability is common to all items and cancels in z, so it is not applied."""
    deg = np.asarray(items_D, np.float64).reshape(-1)
    if not (np.isfinite(deg).all() and (deg > 0).all()):
        raise ValueError("--inbatch_logq 1: the item degrees must be finite and > 0 (the loader sets empty items to 1)")
    return np.log(deg).astype(np.float32)


def resolve_inbatch_mix(config, loss_kind):
    """--inbatch_mix 0 | 1 -> bool.  An option of --loss inbatch: LgcnError naming the flag under any other loss;
    ValueError for a value that is neither."""
    mix = str(config.get('inbatch_mix', 0)).strip().lower()
    if mix not in ('0', '1', 'false', 'true'):
        raise ValueError(f"--inbatch_mix must be 0 or 1, got {config.get('inbatch_mix')!r}")
    mix = mix in ('1', 'true')
    if mix and loss_kind != 'inbatch':
        raise _lib.LgcnError(f"--inbatch_mix 1 is implemented for --loss inbatch only, not for --loss {loss_kind} "
                             "(it adds the sampled negatives to the in-batch score matrix)")
    return mix


_U64 = np.uint64


def _splitmix64(z):
    """splitmix64 of csrc/lgcn_internal.h on NumPy uint64 (arithmetic mod 2^64)."""
    with np.errstate(over='ignore'):
        z = (z + _U64(0x9E3779B97F4A7C15)).astype(np.uint64)
        z = ((z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)).astype(np.uint64)
        z = ((z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)).astype(np.uint64)
        return z ^ (z >> _U64(31))


def hard_neg_rank(seed, step, b, M):
    """The pick j_b of --hard_neg M: lgcn_hn_rank of csrc/lgcn_internal.h restated on NumPy uint64, vectorised over the
    sample indices b -> int64 array in 0..M-1.  step: the Adam step counter BEFORE the step, the convention of the dropout mask."""
    b = np.asarray(b, np.int64)
    with np.errstate(over='ignore'):
        k = _splitmix64((_splitmix64(np.asarray(int(seed) & (2 ** 64 - 1), np.uint64)) + _U64(int(step) & (2 ** 64 - 1))).astype(np.uint64))
        v = _splitmix64(((k ^ _U64(0x4841524E45473031)) + (b & 0xFFFFFFFF).astype(np.uint64)).astype(np.uint64))
    if int(M) <= 1:
        return np.zeros(b.shape, np.int64)
    return ((v >> _U64(32)) % _U64(int(M))).astype(np.int64)


def resolve_hard_neg(config):
    """--hard_neg M -> int in 0..16 (0: off).  ValueError for anything else; what it combines with is LightGCN._refuse_combinations'."""
    try:
        M = int(config.get('hard_neg', 0))
    except (TypeError, ValueError):
        M = -1
    if not 0 <= M <= _lib.MAX_NEG_RATIO:
        raise ValueError(f"--hard_neg must be in 0..{_lib.MAX_NEG_RATIO} (0 = off), got {config.get('hard_neg')!r}")
    return M


def item_logq_mix(items_D, B, R):
    """The logQ vector of --inbatch_logq 1 under --inbatch_mix 1: the log of the expected number of times item i stands among a
    sample's competitors -- (B - 1) in-batch positives drawn in proportion to the train degree and B R pool ids drawn uniformly --
    lq_i = log((B - 1) deg_i / sum deg + B R / m_items), B = --bpr_batch, in float64, rounded once to fp32.  The ragged last
    batch of an epoch uses the same vector."""
    deg = np.asarray(items_D, np.float64).reshape(-1)
    if not (np.isfinite(deg).all() and (deg > 0).all()):
        raise ValueError("--inbatch_logq 1: the item degrees must be finite and > 0 (the loader sets empty items to 1)")
    B, R = int(B), int(R)
    if B < 1 or R < 1:
        raise ValueError(f"--inbatch_mix 1: the batch size and the negative ratio must be >= 1, got {B}, {R}")
    return np.log((B - 1) * deg / deg.sum() + float(B) * R / deg.size).astype(np.float32)


def resolve_layer_weights(config, K, degrees=None):
    """(config, K) -> the fp32 [K+1] weights of out = sum_k w_k X_k, or None for the mean (the reference's combination).
    --layer_weights mean | exp | ppr | "[w_0, ..., w_K]"; the reference's own --use_ppr_weights [--ppr_weights_path FILE]
    (which it parses and never reads) mean `ppr` / the file's row.  degrees: neighbours per node, for a [N, K+1] file."""
    spec = config.get('layer_weights', 'mean')
    spec = 'mean' if spec is None else spec
    named = spec.strip().lower() if isinstance(spec, str) else None
    if config.get('use_ppr_weights', False):
        if named != 'mean':
            raise ValueError(f"--use_ppr_weights and --layer_weights {spec} both name the layer weights: give one of them")
        if config.get('ppr_weights_path', None):
            return load_ppr_weights(config['ppr_weights_path'], K, degrees)
        named = 'ppr'
    k = np.arange(K + 1, dtype=np.float64)
    if named == 'mean':
        return None
    if named == 'exp':
        beta = float(config.get('exp_smooth_beta', 0.5))
        if not (np.isfinite(beta) and beta >= 0.0):
            raise ValueError(f"--layer_weights exp: --exp_smooth_beta must be a finite value >= 0, got {beta}")
        w = beta ** k
        return _check_layer_weights(w / w.sum(), K, "--layer_weights exp")
    if named == 'ppr':
        alpha = float(config.get('ppr_alpha', 0.15))
        if not (0.0 < alpha <= 1.0):
            raise ValueError(f"--layer_weights ppr: --ppr_alpha must be in (0, 1], got {alpha}")
        w = alpha * (1.0 - alpha) ** k
        return _check_layer_weights(w / w.sum(), K, "--layer_weights ppr")
    if named is not None:            # a literal list, taken as written: "[0.4,0.3,0.2,0.1]"
        body = named[1:-1] if named[:1] in '[(' and named[-1:] in '])' else None
        try:
            spec = [float(v) for v in body.split(',')]
        except (ValueError, AttributeError):
            raise ValueError(f"--layer_weights {spec!r}: expected mean, exp, ppr or a list of K + 1 floats") from None
    return _check_layer_weights(spec, K, "--layer_weights")


class _Propagate(torch.autograd.Function):
    """computer() with autograd: forward = lgcn_propagate_mean / _weighted, backward = the Horner
    chain sum_k w_k A^k g (w_k = 1/(K+1) without --layer_weights) through lgcn_spmm_csr (A_hat is symmetric)."""

    @staticmethod
    def forward(ctx, user_w, item_w, model):
        ctx.model = model
        return model._propagate_dense()

    @staticmethod
    def backward(ctx, grad_out):
        m = ctx.model
        if m.layer_weights is not None:      # h_K = w_K G, h_{k-1} = w_{k-1} G + A h_k: the chain of the fused step
            w = [float(v) for v in m.layer_weights]
            g = grad_out.contiguous().float()
            h = w[m.n_layers] * g
            for k in range(m.n_layers, 0, -1):
                h = w[k - 1] * g + m._spmm(h)
            return h[:m.n_users], h[m.n_users:], None
        g = (grad_out.contiguous().float() / float(m.n_layers + 1))
        h = g
        for _ in range(m.n_layers):
            h = g + m._spmm(h)
        return h[:m.n_users], h[m.n_users:], None


class _I2ISmooth(torch.autograd.Function):
    """model.py:228-229: items + alpha * (I2I @ items); backward g + alpha * (I2I^T @ g)."""

    @staticmethod
    def forward(ctx, items, model):
        ctx.model = model
        return model._i2i_apply(items, transpose=False)

    @staticmethod
    def backward(ctx, grad):
        return ctx.model._i2i_apply(grad, transpose=True), None


class _TableModel(nn.Module):
    """What LightGCN and PureMF share: the two embedding tables as views of ONE contiguous [N, d] fp32 table (rows [0, n_users)
    the users), the device state `_dev` with its training context, and the host side of a fused step or epoch around its C call.

    The two context types differ in the names of their entry points, `_CTX`; a subclass adds what is its own: how a context is
    built (`_make_ctx`, from the pieces below), when one is stale (`_ctx_stale`), what else its device state holds
    (`_open_state`, `_ctx_rows`, `_close_state`), which entry point a batch goes to (`_dispatch`) and what it memoises
    (`invalidate_cache`)."""
    _CTX = None     # {'destroy', 'get_step', 'set_step', 'set_lr', 'check', 'step', 'epoch'} -> entry point of the context type

    def __init__(self, config, dataset):
        super().__init__()
        self.config = config
        self.dataset = dataset
        self.device = world.device
        self.n_users = dataset.n_users
        self.m_items = dataset.m_items
        self.latent_dim = config['latent_dim_rec']

    # -- config keys that are read when they are needed, not at construction (tests and BPRLoss assign them later) --
    def _act(self):
        return str(self.config.get('act_dtype', 'fp32'))

    def _reg_ego(self):
        return str(self.config.get('reg_rows', 'propagated')) == 'ego'

    def _batch(self, default):
        return int(self.config.get('bpr_batch_size', default))

    # -- parameters live in one table ------------------------------------------------
    def _bind_table(self):
        """The two freshly initialised nn.Embedding weights move into ONE contiguous [N, d] storage (the cat of model.py:209
        becomes a no-op)."""
        with torch.no_grad():
            table = torch.cat([self.embedding_user.weight, self.embedding_item.weight], dim=0).contiguous()
        self._table = table
        self._rebind()
        self._dev = None            # device-side state (graph, workspace, context)

    def _rebind(self):
        self.embedding_user.weight.data = self._table[:self.n_users]
        self.embedding_item.weight.data = self._table[self.n_users:]

    def _apply(self, fn, recurse=True):
        # keep the single-storage invariant through .to()/.cuda()/.float()
        new = fn(self._table)
        if new is not self._table:
            self._table = new
            self._drop_device_state()
        self._rebind()
        for p in (self.embedding_user.weight, self.embedding_item.weight):
            if p.grad is not None:
                p.grad = fn(p.grad)
        return self

    def _check_table(self):
        """state_dict loads and optimisers write through the parameter views; make sure
        nobody replaced them by independent tensors."""
        u, i = self.embedding_user.weight, self.embedding_item.weight
        if (u.data_ptr() != self._table.data_ptr()
                or i.data_ptr() != self._table.data_ptr() + self.n_users * self.latent_dim * 4):
            with torch.no_grad():
                self._table[:self.n_users].copy_(u.data)
                self._table[self.n_users:].copy_(i.data)
            self._rebind()

    # -- device state -----------------------------------------------------------------
    def invalidate_cache(self):
        """Hook probed by main.py:190-191 before each Test; here nothing is cached."""

    def _open_state(self):
        return {'ctx': None, 'max_batch': 0}

    def _ctx_rows(self, st, row_subset):
        return 'all'

    def _close_state(self, st):
        pass

    def _retire_ctx(self, st):
        """Destroys the context of st, if any -> its Adam step counter (0 without one), which the next context takes over."""
        if not st.get('ctx'):
            return 0
        lib = _lib.load()
        step = getattr(lib, self._CTX['get_step'])(st['ctx'])
        getattr(lib, self._CTX['destroy'])(st['ctx'])
        st['ctx'] = None
        return step

    def _drop_device_state(self):
        st = self._dev
        if st is not None:
            self._retire_ctx(st)
            self._close_state(st)
        self._dev = None
        self.invalidate_cache()

    def __del__(self):
        try:
            self._drop_device_state()
        except Exception:
            pass

    def _state(self, max_batch=None, need_ctx=False, dp_world=1, row_subset=None):
        _lib.require_gpu()
        if not self._table.is_cuda:
            raise _lib.LgcnError("model parameters are not on the GPU: call .to(world.device) first")
        self._check_table()
        if self._dev is None:
            self._dev = self._open_state()
        st = self._dev
        rows = 'all' if row_subset is None else self._ctx_rows(st, row_subset)
        if need_ctx:
            max_batch = int(max_batch or self._batch(2048))
            if st['ctx'] is None or st['max_batch'] < max_batch or self._ctx_stale(st, dp_world, rows):
                self._make_ctx(max_batch, dp_world, rows)
        return st

    # -- the pieces of _make_ctx both context types use ---------------------------------------
    def _step_workspace(self, st, n_terms):
        """Adam's moments (kept over a rebuild) and what one step accumulates in: G64, the row bitmaps, n_terms loss / reg terms,
        the error flag (a step leaves G64 all zero and one bitmap flagged; a new context starts on fresh ones)."""
        N, d, dev = self.n_users + self.m_items, self.latent_dim, self._table.device
        if 'adam_m' not in st:
            st['adam_m'] = torch.zeros(N, d, dtype=torch.float32, device=dev)
            st['adam_v'] = torch.zeros(N, d, dtype=torch.float32, device=dev)
        st['G64'] = torch.zeros(N, d, dtype=torch.int64, device=dev)
        st['bitmap'] = torch.zeros(2 * ((N + 31) // 32), dtype=torch.int32, device=dev)
        st['terms'] = torch.zeros(n_terms, dtype=torch.float32, device=dev)
        st['err'] = torch.zeros(1, dtype=torch.int32, device=dev)

    def _fill_step_config(self, cfg, st, max_batch):
        """The fields lgcn_train_config and lgcn_mf_config share: sizes, the table, _step_workspace's buffers, Adam's constants."""
        cfg.n_users, cfg.d = self.n_users, self.latent_dim
        cfg.E0, cfg.adam_m, cfg.adam_v = self._table.data_ptr(), st['adam_m'].data_ptr(), st['adam_v'].data_ptr()
        cfg.G64, cfg.bitmap, cfg.terms = st['G64'].data_ptr(), st['bitmap'].data_ptr(), st['terms'].data_ptr()
        cfg.err, cfg.max_batch = st['err'].data_ptr(), max_batch
        cfg.decay = float(self.config.get('decay', 1e-4))
        cfg.lr = float(self.config.get('lr', 1e-3))
        cfg.beta1, cfg.beta2, cfg.eps = 0.9, 0.999, 1e-8
        return cfg

    def _create_ctx(self, create, cfg, setters):
        """`create`(cfg) -> the context handle, after every (entry, args) of `setters` was applied to it in order.  A setter that
        fails destroys the new context (it holds device allocations) and its error goes on."""
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(getattr(lib, create)(C.byref(cfg), C.byref(h)), create)
        try:
            for entry, args in setters:
                _lib.check(getattr(lib, entry)(h, *args) or 0, entry)      # (set_step returns nothing: it cannot fail)
        except Exception:
            getattr(lib, self._CTX['destroy'])(h)
            raise
        return h

    # -- fused path (what BPRLoss.stageOne calls) ------------------------------------------
    @staticmethod
    def _ids(t, dev):
        if not torch.is_tensor(t):
            t = torch.as_tensor(np.asarray(t))
        return t.to(device=dev, dtype=torch.int32).contiguous()

    def _dispatch(self, users, pos, neg, batch_size=None):
        """A step's batch (batch_size None) or an epoch's id arrays -> (entry point, its arguments between the context and the
        output, number of samples, the converted id tensors: the caller holds them until the call has been made).  Here: the
        three-slot form, one negative per positive."""
        dev = self._table.device
        held = users, pos, neg = self._ids(users, dev), self._ids(pos, dev), self._ids(neg, dev)
        T = int(users.numel())
        if batch_size is None:
            return self._CTX['step'], (_lib.tp(users), _lib.tp(pos), _lib.tp(neg), T), T, held
        return self._CTX['epoch'], (_lib.tp(users), _lib.tp(pos), _lib.tp(neg), T, int(batch_size)), T, held

    def _dp_begin(self, users, pos, neg, lr, dp_world, global_batch=None, row_subset=None):
        """parallel.DataParallelBPR's preamble of a step on the given samples, or of an epoch over them in global batches:
        int32 ids, the state for max(B, --bpr_batch) (B the step's or the global batch) and this world size, the learning
        rate, the output -> (users, pos, neg, state, loss_out [3] or [steps, 3])."""
        dev = self._table.device
        users, pos, neg = self._ids(users, dev), self._ids(pos, dev), self._ids(neg, dev)
        T = int(users.numel())
        B = global_batch or T
        st = self._state(max_batch=max(B, self._batch(B)), need_ctx=True, dp_world=dp_world, row_subset=row_subset)
        getattr(_lib.load(), self._CTX['set_lr'])(st['ctx'], float(lr))
        loss = torch.empty(((T + B - 1) // B, 3) if global_batch else 3, dtype=torch.float32, device=dev)
        return users, pos, neg, st, loss

    def _fused_call(self, entry, args, T, batch_size=None, loss_out=None, lr=None):
        """What every fused step and epoch does around its C call: the state for max_batch (an epoch's batch_size; a step's T, or
        --bpr_batch if that is larger), the learning rate, the output -- loss_out [3] of a step, [steps, 3] of an epoch --,
        `entry`(ctx, *args, output, stream), its check, the cache.  args: the entry point's arguments between the context and
        the output, or a function of the state that returns them.  Returns the output."""
        dev = self._table.device
        epoch = batch_size is not None
        st = self._state(max_batch=batch_size if epoch else max(T, self._batch(T)), need_ctx=True,
                         dp_world=(self._dev or {}).get('dp_world', 1))
        lib = _lib.load()
        if lr is not None:
            getattr(lib, self._CTX['set_lr'])(st['ctx'], float(lr))
        if epoch:
            loss_out = torch.empty((T + batch_size - 1) // batch_size, 3, dtype=torch.float32, device=dev)
        elif loss_out is None:
            loss_out = torch.empty(3, dtype=torch.float32, device=dev)
        if callable(args):
            args = args(st)
        _lib.check(getattr(lib, entry)(st['ctx'], *args, _lib.tp(loss_out), _lib.current_stream()), entry.replace("_i64", ""))
        self.invalidate_cache()
        return loss_out

    def fused_step(self, users, pos, neg, loss_out=None, lr=None):
        """One BPRLoss.stageOne (utils.py:53-64) in the HIP kernels.  Returns a device
        tensor [3] = (bpr + decay*reg, bpr, reg); no host synchronisation."""
        entry, args, B, held = self._dispatch(users, pos, neg)
        return self._fused_call(entry, args, B, None, loss_out, lr)

    def fused_epoch(self, users, pos, neg, batch_size, lr=None):
        """The loop of main.py:223-225 over already-shuffled device id arrays, one C call.
        Returns a device tensor [steps,3] of per-step (loss, bpr, reg)."""
        entry, args, T, held = self._dispatch(users, pos, neg, int(batch_size))
        return self._fused_call(entry, args, T, int(batch_size), None, lr)

    def check_device_errors(self):
        if self._dev and self._dev.get('ctx'):
            _lib.check(getattr(_lib.load(), self._CTX['check'])(self._dev['ctx'], _lib.current_stream()), "device id check")

    @property
    def adam_step(self):
        return getattr(_lib.load(), self._CTX['get_step'])(self._dev['ctx']) if self._dev and self._dev.get('ctx') else 0

    def set_adam_step(self, step):
        """torch Adam's state['step'] of a loaded optimizer state -> the training context (made if need be)."""
        getattr(_lib.load(), self._CTX['set_step'])(self._state(need_ctx=True)['ctx'], int(step))


class LightGCN(_TableModel):
    _CTX = {'destroy': 'lgcn_ctx_destroy', 'get_step': 'lgcn_ctx_get_step', 'set_step': 'lgcn_ctx_set_step', 'set_lr': 'lgcn_ctx_set_lr',
            'check': 'lgcn_ctx_check', 'step': 'lgcn_train_step', 'epoch': 'lgcn_train_epoch'}

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.n_layers = config['lightGCN_n_layers']
        # edge dropout (upstream LightGCN's __dropout_x; --dropout 1 --keepprob p): the fused training step draws one mask per
        # optimiser step (lgcn_ctx_set_dropout); evaluation never drops
        self.dropout = bool(config.get('dropout', 0))
        self.keep_prob = float(config.get('keep_prob', 0.6))
        if self.dropout and not (0.0 < self.keep_prob <= 1.0):
            raise ValueError(f"--keepprob must be in (0, 1] with --dropout 1, got {self.keep_prob}")
        if self.latent_dim not in (32, 64, 128, 256):
            raise ValueError("latent_dim_rec must be 32, 64, 128 or 256 for the HIP kernels")
        if not (1 <= self.n_layers <= _lib.MAX_LAYERS):
            raise ValueError(f"lightGCN_n_layers must be in 1..{_lib.MAX_LAYERS}")

        # Same RNG consumption as model.py:57-60 (two nn.Embedding ctors, then two normal_),
        # then both tables are moved into ONE contiguous [N,d] storage: rows [0,n_users) are
        # embedding_user.weight, rows [n_users,N) embedding_item.weight.
        self.embedding_user = nn.Embedding(self.n_users, self.latent_dim)
        self.embedding_item = nn.Embedding(self.m_items, self.latent_dim)
        nn.init.normal_(self.embedding_user.weight, std=0.1)
        nn.init.normal_(self.embedding_item.weight, std=0.1)
        self._bind_table()

        # popularity gate (model.py:66-96): same modules, built in the same order -> same initial weights
        self.use_pop_gate = bool(config.get('use_pop_gate', False))
        self.pop_hidden = int(config.get('pop_hidden', 32))
        self.gate_hidden = int(config.get('gate_hidden', 64))
        self.gate_entropy_coeff = float(config.get('gate_entropy_coeff', 1e-4))
        self.pop_gate_temp = float(config.get('pop_gate_temp', 1.0))
        if self.use_pop_gate:
            counts = torch.clamp(torch.from_numpy(np.asarray(dataset.items_D)).float(), min=0.0)
            pop = torch.log1p(counts)
            self.item_pop_scalar = (pop - pop.mean()) / (pop.std() + 1e-8)
            self.pop_mlp = nn.Sequential(nn.Linear(1, self.pop_hidden), nn.ReLU(), nn.Linear(self.pop_hidden, self.latent_dim))
            self.gate_mlp = nn.Sequential(nn.Linear(self.latent_dim * 2, self.gate_hidden), nn.ReLU(), nn.Linear(self.gate_hidden, 1))
        else:
            self.item_pop_scalar, self.pop_mlp, self.gate_mlp = None, None, None

        # item-item graph (model.py:99-109): a CSR [m_items, m_items] from an .npz; unreadable -> warning, off
        self.use_item_item = bool(config.get('use_item_item', False))
        self.i2i_alpha = float(config.get('i2i_alpha', 0.0))
        self._i2i = None
        if self.use_item_item and config.get('i2i_path', None):
            try:
                import scipy.sparse as sp
                m = sp.load_npz(config['i2i_path']).tocsr().astype(np.float32)
                if m.shape != (self.m_items, self.m_items):
                    raise ValueError(f"shape {m.shape} is not ({self.m_items}, {self.m_items})")
                m.sort_indices()
                self._i2i = m
                world.cprint(f"[I2I] loaded {config['i2i_path']}, nnz={m.nnz}")
            except Exception as e:      # noqa: BLE001 -- the reference warns and goes on without it
                world.cprint(f"[I2I] WARNING: cannot load {config['i2i_path']}: {e}")
        elif self.use_item_item and config.get('i2i_build', 'none') not in (None, 'none'):
            # NEW: no file given -- the graph the reference's preprocess_instacart_i2i.py would have written, built on the GPU
            # from the train baskets (one per user with train items, in user order).  A failure here is an error, not a warning.
            from . import preprocess_instacart_i2i as i2i
            r = dataset.UserItemNet.tocsr()
            sizes = np.diff(r.indptr)
            keep = sizes > 0
            indptr = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int64)
            self._i2i = i2i.build_from_csr(indptr, r.indices, self.m_items, topk=int(config.get('i2i_topk', 50)),
                                           weight=config['i2i_build'], min_basket=int(config.get('i2i_min_basket', 1)))
            world.cprint(f"[I2I] built {config['i2i_build']} topk={int(config.get('i2i_topk', 50))} on the GPU, nnz={self._i2i.nnz}")

        self._adj = dataset.getSparseGraphCSR() if hasattr(dataset, 'getSparseGraphCSR') else None
        if self._adj is None:                       # generic BasicDataset: COO -> CSR
            g = dataset.getSparseGraph().coalesce().cpu()
            import scipy.sparse as sp
            idx = g.indices().numpy()
            self._adj = sp.csr_matrix((g.values().numpy().astype(np.float32), (idx[0], idx[1])),
                                      shape=tuple(g.shape))
            self._adj.sort_indices()
        N = self.n_users + self.m_items
        if self._adj.shape != (N, N):
            raise ValueError("adjacency shape does not match n_users + m_items")
        if len(self._adj.indices) and (self._adj.indices.min() < 0 or self._adj.indices.max() >= N):
            raise ValueError("adjacency column index out of range")
        # weights of the layer combination (--layer_weights, --use_ppr_weights): fp32 [K+1], or None = the reference's mean.
        # The fused step (lgcn_ctx_set_layer_weights), the autograd path and evaluation (lgcn_propagate_weighted) all use them
        self.layer_weights = resolve_layer_weights(config, self.n_layers, np.diff(self._adj.indptr))
        # several negatives per positive (--neg_ratio R; lgcn_train_step_multi): the default model, fp32 / bf16 storage
        self.neg_ratio = int(config.get('neg_ratio', 1))
        if not 1 <= self.neg_ratio <= _lib.MAX_NEG_RATIO:
            raise ValueError(f"--neg_ratio must be in 1..{_lib.MAX_NEG_RATIO}, got {self.neg_ratio}")
        # the loss of the fused step (--loss bpr | softmax, --softmax_temp; lgcn_ctx_set_loss): softmax = the positive
        # against all R negatives of its sample in one log-sum-exp; every negative shape then goes to the _multi entry points.
        # inbatch = every user of the batch against every positive of the batch; the sampled negatives are not used
        # directau = alignment of the samples' two rows and uniformity of the batch's users and of its items, on the
        # rows over their norms, weight --au_gamma; no negatives at all
        self.loss_kind, self.softmax_temp = resolve_loss(config)
        self.au_gamma = resolve_au_gamma(config, self.loss_kind)
        # hard negatives (--hard_neg M; lgcn_ctx_set_hard_neg): the multi-negative step trains the BPR triplet on one of the
        # M hardest of its R candidates.  hard_neg_step: the step counter bpr_loss keys its picks with (None: adam_step, the fused
        # step's own convention -- the counter before the step)
        self.hard_neg = resolve_hard_neg(config)
        self.hard_neg_step = None
        # mixed negatives (--inbatch_mix 1; lgcn_train_step_inbatch_mix): the sampled negatives of the batch as shared
        # extra columns of the in-batch score matrix; --neg_ratio 1..16 is then legal.  Resolved among the refusals, where its own lie
        self.inbatch_mix = self._refuse_combinations()
        self._neg_ratio_said = self._loss_said = False      # (_ctx_dense_last says each of its two lines once)
        # the two options of the in-batch step (--score dot | cosine, --inbatch_logq 0 | 1; lgcn_ctx_set_inbatch_scores)
        self.score_kind, self.inbatch_logq = resolve_inbatch_scores(config, self.loss_kind)
        self._item_logq = None      # fp32 [m_items] log(items_D), rounded once from float64 (None: --inbatch_logq 0)
        if self.inbatch_logq and self.inbatch_mix:      # the log of the mixture's expected count
            self._item_logq = torch.from_numpy(item_logq_mix(dataset.items_D, self._batch(2048), self.neg_ratio))
        elif self.inbatch_logq:
            self._item_logq = torch.from_numpy(item_logq(dataset.items_D))
        self._gate_flat = None      # the eight MLP tensors of the gate in ONE buffer (what the fused step reads / updates)
        self._Graph = None
        self._cache = None          # propagated embeddings memoised between invalidate_cache() calls
        self._rating_cache = None
        self._cosine_cache = None   # --score cosine: the row-normalised propagated table evaluation ranks with, memoised likewise
        self.f = nn.Sigmoid()

    def _refuse_combinations(self):
        """The pairs of options no launch exists for, first match first: --hard_neg, storage, optional branches, dropout, layer weights,
        --neg_ratio, --loss, --inbatch_mix -> the resolved --inbatch_mix, whose own refusals (resolve_inbatch_mix) stand between
        those of the loss and the last one.  (A value that is invalid on its own was refused where it was read, before all these.)"""
        config = self.config
        fp8 = self._act() == 'fp8'
        if self.hard_neg:       # first: every one of these names --hard_neg (with it off nothing here is reached)
            M, R = self.hard_neg, self.neg_ratio
            if R < 2:
                raise _lib.LgcnError(f"--hard_neg {M} needs --neg_ratio >= 2 (the candidates it picks among), got --neg_ratio {R}")
            if M > R:
                raise _lib.LgcnError(f"--hard_neg {M} exceeds --neg_ratio {R}: the pick is among the M hardest of R candidates, M <= R")
            if self.loss_kind != 'bpr':
                raise _lib.LgcnError(f"--hard_neg {M} is implemented for --loss bpr only, not for --loss {self.loss_kind} "
                                     "(the selected triplet trains the BPR loss)")
            if fp8:
                raise _lib.LgcnError(f"--hard_neg {M} is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)")
            if self.use_pop_gate:
                raise _lib.LgcnError(f"--hard_neg {M} is not implemented together with --use_pop_gate (the popularity gate trains on one "
                                     "sampled negative per positive)")
            if self.use_item_item:
                raise _lib.LgcnError(f"--hard_neg {M} is not implemented together with --use_item_item (the item-item smoothing trains on "
                                     "one sampled negative per positive)")
        if self.dropout and fp8:
            raise _lib.LgcnError("--dropout 1 is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)")
        if self.dropout and self.has_variants:
            raise _lib.LgcnError("--dropout 1 is not implemented together with --use_pop_gate / --use_item_item "
                                 "(the popularity gate and the item-item smoothing train without edge dropout only)")
        if self.layer_weights is not None:
            flag = "--use_ppr_weights" if config.get('use_ppr_weights', False) else "--layer_weights"
            if fp8:
                raise _lib.LgcnError(f"{flag} is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)")
            if self.has_variants:
                raise _lib.LgcnError(f"{flag} is not implemented together with --use_pop_gate / --use_item_item "
                                     "(the optional branches train with the layer mean only)")
            if self.dropout:
                raise _lib.LgcnError(f"{flag} is not implemented together with --dropout 1 (edge dropout trains with the layer mean only)")
        if self.neg_ratio > 1:
            if fp8:
                raise _lib.LgcnError(f"--neg_ratio {self.neg_ratio} is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)")
            if self.use_pop_gate or self.use_item_item:
                raise _lib.LgcnError(f"--neg_ratio {self.neg_ratio} is not implemented together with --use_pop_gate / --use_item_item "
                                     "(the optional branches train on one negative per positive)")
        if self.loss_kind != 'bpr':
            if fp8:
                raise _lib.LgcnError(f"--loss {self.loss_kind} is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)")
            if self.use_pop_gate or self.use_item_item:
                raise _lib.LgcnError(f"--loss {self.loss_kind} is not implemented together with --use_pop_gate / --use_item_item "
                                     "(the optional branches train with the BPR loss only)")
        mix = resolve_inbatch_mix(config, self.loss_kind)
        if self.loss_kind == 'inbatch' and self.neg_ratio > 1 and not mix:
            raise _lib.LgcnError(f"--loss inbatch is not implemented together with --neg_ratio {self.neg_ratio}: the in-batch loss has no "
                                 "sampled negatives (the other samples' positives are the negatives); use --neg_ratio 1")
        if self.loss_kind == 'directau' and self.neg_ratio > 1:
            raise _lib.LgcnError(f"--loss directau is not implemented together with --neg_ratio {self.neg_ratio}: the alignment-and-"
                                 "uniformity loss has no negatives at all; use --neg_ratio 1")
        return mix

    # -- parameters live in one table: the gate's tensors follow it ----------------------
    def _apply(self, fn, recurse=True):
        super()._apply(fn)
        for mod in (self.pop_mlp, self.gate_mlp):
            if mod is not None:
                mod._apply(fn)
        if self.item_pop_scalar is not None:
            self.item_pop_scalar = fn(self.item_pop_scalar)
        return self

    def _check_table(self):
        super()._check_table()
        if self.use_pop_gate:
            self._pack_gate()

    def gate_parameters(self):
        """The gate's eight tensors in torch's named_parameters order (pop_mlp.0.weight ... gate_mlp.2.bias)."""
        return list(self.pop_mlp.parameters()) + list(self.gate_mlp.parameters())

    def _pack_gate(self):
        """The fused step reads and updates the gate's MLPs as ONE fp32 buffer (include/lgcn_hip.h: gate_params): keep the
        nn.Linear parameters views of it.  Returns True when the buffer was (re)made -- a context bound to the old one is stale."""
        ps = self.gate_parameters()
        flat, off, ok = self._gate_flat, 0, self._gate_flat is not None
        for prm in ps:
            ok = ok and prm.device == flat.device and prm.data_ptr() == flat.data_ptr() + 4 * off and prm.is_contiguous()
            off += prm.numel()
        if ok:
            return False
        flat = torch.cat([prm.data.reshape(-1).float() for prm in ps]).contiguous()
        off = 0
        for prm in ps:
            prm.data = flat[off:off + prm.numel()].view(prm.shape)
            off += prm.numel()
        self._gate_flat = flat
        if self._dev is not None and self._dev.get('ctx'):
            _lib.load().lgcn_ctx_destroy(self._dev['ctx'])
            self._dev['ctx'] = None
        return True

    @property
    def fused_variants(self):
        """The optional branches run inside the fused HIP step (default) unless --fused_variants 0 asks for the autograd
        path or the gate's shape is outside what k_triplet_gate holds in LDS (hidden sizes <= 64, d <= 128)."""
        if not self.has_variants:
            return False
        if not int(self.config.get('fused_variants', 1)):
            return False
        if self.use_pop_gate and (self.latent_dim > 128 or self.pop_hidden > 64 or self.gate_hidden > 64 or self.pop_gate_temp <= 0):
            return False
        return True

    @property
    def Graph(self):
        """torch sparse COO of A_hat as the reference keeps it (model.py:63); built lazily."""
        if self._Graph is None:
            self._Graph = self.dataset.getSparseGraph()
        return self._Graph

    # -- device state -----------------------------------------------------------------
    def _close_state(self, st):
        for key in ('graph_rs', 'graph', 'i2i', 'i2i_t', 'i2i_s', 'i2i_ts'):
            if st.get(key) is not None:
                st[key].close()

    def _open_state(self):
        a, dev = self._adj, self._table.device
        from . import reorder
        order, xcd_start = reorder.row_order(self.config.get('row_order', 'natural'), self.dataset, a,
                                             cache_dir=getattr(self.dataset, 'path', None))
        return {
            'graph': _lib.Graph(torch.from_numpy(np.ascontiguousarray(a.indptr, np.int32)).to(dev),
                                torch.from_numpy(np.ascontiguousarray(a.indices, np.int32)).to(dev),
                                torch.from_numpy(np.ascontiguousarray(a.data, np.float32)).to(dev),
                                d_max=self.latent_dim, row_order=order, xcd_start=xcd_start),
            'ctx': None, 'max_batch': 0,
        }

    def _ctx_rows(self, st, row_subset):
        """A context is bound to ONE plan: the owned rows (row-sharded epochs, which exchange the other rows: a row_subset is
        given, and this is called) or all rows (every other caller: fused_step / fused_epoch / stageOne / batch-sharded data
        parallel).  Makes the plan of the owned rows -> 'owned'."""
        if st.get('graph_rs') is None:
            # row-sharded propagation: the training context works on a plan of the owned rows only
            # (same device CSR arrays); evaluation keeps the full plan
            g = st['graph']
            st['graph_rs'] = _lib.Graph(g.indptr, g.indices, g.vals, d_max=self.latent_dim,
                                        row_order=np.ascontiguousarray(row_subset, np.int32))
        return 'owned'

    def _ctx_stale(self, st, dp_world, rows):
        # a context made for one plan must not serve the other -- it would propagate over the owned rows only, with no exchange
        return st.get('dp_world', 1) != dp_world or st.get('ctx_rows', 'all') != rows

    def _make_ctx(self, max_batch, dp_world, rows=None):
        st = self._dev
        old_step = self._retire_ctx(st)
        rows = rows or st.get('ctx_rows', 'all')
        variants, act_dtype = self.fused_variants, _act_code(self._act())
        dense_last = self._ctx_dense_last(max_batch, variants)
        self._ctx_workspace(st, max_batch, dp_world, dense_last, variants, act_dtype)
        cfg = self._ctx_config(st, max_batch, rows, dense_last, variants, act_dtype)
        st['ctx'] = self._create_ctx('lgcn_ctx_create', cfg, self._ctx_setters(st, old_step))
        st['max_batch'], st['dp_world'], st['table_ptr'], st['ctx_rows'] = max_batch, dp_world, self._table.data_ptr(), rows
        st['dense_last'] = dense_last

    def _ctx_dense_last(self, max_batch, variants):
        """Is the last forward layer propagated densely?  _dense_last on the configured batch (not this context's capacity), and
        always where the step has no gathered form: the optional branches, --neg_ratio > 1, a loss other than BPR."""
        dense_last = self._dense_last(self._batch(max_batch))
        if variants:
            dense_last = True       # the optional branches score on the layer mean of EVERY row (model.py:221-229)
        if self.neg_ratio > 1 and not dense_last:
            dense_last = True       # the 2 + R slot batch-row kernel reads a dense last layer (the gathered form is not built)
            if not self._neg_ratio_said:
                world.cprint(f"[neg_ratio] --neg_ratio {self.neg_ratio}: the last layer is propagated densely (dense_last = 1)")
                self._neg_ratio_said = True
        if self.loss_kind != 'bpr' and not dense_last:
            dense_last = True       # the softmax batch-row kernel is the 2 + R slot form too, the in-batch and directau launches their 2 B slot form
            if not self._loss_said:
                world.cprint(f"[loss] --loss {self.loss_kind}: the last layer is propagated densely (dense_last = 1)")
                self._loss_said = True
        return dense_last

    def _ctx_workspace(self, st, max_batch, dp_world, dense_last, variants, act_dtype):
        """Every device buffer and graph a context for max_batch reads or writes, into st."""
        N, d, K, dev = self.n_users + self.m_items, self.latent_dim, self.n_layers, self._table.device
        self._step_workspace(st, 3 * max_batch)
        st['act'] = _act_tables(max(1, K if dense_last else K - 1), N, d, act_dtype, dev)
        shard = (max_batch + dp_world - 1) // dp_world
        gate_p = sum(prm.numel() for prm in self.gate_parameters()) if (variants and self.use_pop_gate) else 0
        # exchange block of a rank (lgcn_dp_block_floats): gradient rows, loss / reg (/ entropy) terms, the gate's fixed-point MLP sums
        st['contrib'] = torch.zeros(3 * shard * d + 3 * shard + 2 + 2 * gate_p, dtype=torch.float32, device=dev)
        # config['hard_neg_record'] = 1 (tests): the steps store the selected index of every sample here (last_selection)
        st['hard_neg_sel'] = (torch.full((max_batch,), -1, dtype=torch.int32, device=dev)
                              if self.hard_neg and int(self.config.get('hard_neg_record', 0)) else None)
        if self.inbatch_logq and (st.get('item_logq') is None or st['item_logq'].device != dev):
            st['item_logq'] = self._item_logq.to(device=dev, dtype=torch.float32).contiguous()      # uploaded once
        if variants and self.i2i_active:
            # the fused step's graphs hold alpha * I2I and its transpose (model.py:228-229 scales after the product)
            for key, mat in (('i2i_s', self._i2i), ('i2i_ts', self._i2i.T.tocsr())):
                if key not in st:
                    mat = mat.tocsr().astype(np.float32)
                    mat.sort_indices()
                    st[key] = _lib.Graph(torch.from_numpy(mat.indptr.astype(np.int32)).to(dev), torch.from_numpy(mat.indices.astype(np.int32)).to(dev),
                                         torch.from_numpy((np.float32(self.i2i_alpha) * mat.data).astype(np.float32)).to(dev), d_max=d)
        if variants and self.use_pop_gate:
            self._pack_gate()
            P = self._gate_flat.numel()
            for key in ('gate_m', 'gate_v', 'gate_grad'):
                if key not in st or st[key].numel() != P:
                    st[key] = torch.zeros(P, dtype=torch.float32, device=dev)
            st['item_pop'] = self.item_pop_scalar.to(device=dev, dtype=torch.float32).contiguous()

    def _ctx_config(self, st, max_batch, rows, dense_last, variants, act_dtype):
        """-> lgcn_train_config over the buffers of _ctx_workspace."""
        cfg = self._fill_step_config(_lib.TrainConfig(), st, max_batch)
        cfg.graph = (st['graph_rs'] if rows == 'owned' else st['graph']).handle
        cfg.K, cfg.act_dtype = self.n_layers, act_dtype
        cfg.act, cfg.contrib = st['act'].data_ptr(), st['contrib'].data_ptr()
        cfg.reg_ego = int(self._reg_ego())
        if cfg.reg_ego and variants:
            raise _lib.LgcnError("--reg_rows ego (upstream LightGCN's L2 term) is defined for the default model, not with "
                                 "--use_pop_gate / --use_item_item")
        cfg.xcd_remap = int(self.config.get('xcd_remap', 1))
        cfg.dense_last = int(dense_last)
        cfg.hub_nnz = int(self.config.get('hub_nnz', 0))          # 0: library default; < 0: off
        cfg.hub_chunk = int(self.config.get('hub_chunk', 0))
        if variants and self.i2i_active:
            cfg.i2i, cfg.i2i_t = st['i2i_s'].handle, st['i2i_ts'].handle
        if variants and self.use_pop_gate:
            cfg.item_pop, cfg.gate_params = st['item_pop'].data_ptr(), self._gate_flat.data_ptr()
            cfg.gate_adam_m, cfg.gate_adam_v, cfg.gate_grad = st['gate_m'].data_ptr(), st['gate_v'].data_ptr(), st['gate_grad'].data_ptr()
            cfg.pop_hidden, cfg.gate_hidden = self.pop_hidden, self.gate_hidden
            cfg.gate_entropy_coeff, cfg.pop_gate_temp = self.gate_entropy_coeff, self.pop_gate_temp
        return cfg

    def _ctx_setters(self, st, old_step):
        """-> [(entry point, its arguments after the context)] in the order they are applied.  Each option is set only when it is
        on: a context that is never told keeps the workspace and runs the launches it always had."""
        out = [('lgcn_ctx_set_step', (old_step,))]
        if self.dropout:
            out.append(('lgcn_ctx_set_dropout', (self.keep_prob, int(self.config.get('seed', 2020)) & (2 ** 64 - 1))))
        if self.layer_weights is not None:
            w = np.ascontiguousarray(self.layer_weights, dtype=np.float32)      # (the pointer object keeps it alive until it is applied)
            out.append(('lgcn_ctx_set_layer_weights', (_lib.npp(w), int(w.size))))
        if self.loss_kind == 'directau':
            out.append(('lgcn_ctx_set_directau', (float(self.au_gamma),)))
        elif self.loss_kind != 'bpr':
            out.append(('lgcn_ctx_set_loss', (_lib.LOSS_INBATCH if self.loss_kind == 'inbatch' else _lib.LOSS_SOFTMAX, float(self.softmax_temp))))
        if self.score_kind != 'dot' or self.inbatch_logq:
            out.append(('lgcn_ctx_set_inbatch_scores', (_lib.SCORE_COSINE if self.score_kind == 'cosine' else _lib.SCORE_DOT,
                                                        _lib.tp(st['item_logq']) if self.inbatch_logq else None)))
        if self.inbatch_mix:
            out.append(('lgcn_ctx_set_inbatch_mix', (int(self.neg_ratio),)))
        if self.hard_neg:
            out.append(('lgcn_ctx_set_hard_neg', (int(self.hard_neg), int(self.config.get('seed', 2020)) & (2 ** 64 - 1),
                                                  _lib.tp(st['hard_neg_sel']) if st.get('hard_neg_sel') is not None else None)))
        if str(self.config.get('fold_g32', 1)).strip().lower() in ('0', 'false', 'off'):      # config['fold_g32'] = 0: fused_epoch launches k_g32 every step again (A/B, tests)
            out.append(('lgcn_ctx_set_fold_g32', (0,)))
        if self.config.get('store_policy') is not None:      # config['store_policy'] = LGCN_STORE_* bits (A/B, tests); unset: LGCN_STORE_POLICY or the library's default
            out.append(('lgcn_ctx_set_store_policy', (int(self.config['store_policy']),)))
        return out

    def _dense_last(self, batch):
        """Last forward layer: on the 3B batch rows only (default) or densely?  The batch rows hold an
        expected  B * (E[deg(user)] + E_pop[deg(item)] + E[deg(item)])  non-zeros -- the positive is drawn
        proportionally to item popularity (sum d^2 / sum d), the negative uniformly.  Per non-zero the
        per-slot gathers cost 2.5-5x what the dense kernel does (measured: Gowalla 17 us at 0.15 nnz(A_hat),
        Yelp-shaped 236 us at 2.1, Amazon-shaped 364 us at 0.34 against dense layers of 29 / 46 / 210 us: a
        slot is one workgroup, and a hub row's tiles are walked serially), so 'auto' goes dense above 0.3
        ('--dense_last 0/1' forces it; the result is the same up to fp32 summation order)."""
        mode = str(self.config.get('dense_last', 'auto'))
        if mode in ('0', '1'):
            return mode == '1'
        deg = np.diff(self._adj.indptr).astype(np.float64)
        du, di = deg[:self.n_users], deg[self.n_users:]
        per_triplet = du.mean() + (di * di).sum() / max(di.sum(), 1.0) + di.mean()
        return bool(batch * per_triplet > 0.3 * self._adj.nnz)

    # -- kernels ------------------------------------------------------------------------
    def _spmm(self, x):
        return self._state()['graph'].spmm(x.float(), _lib.F32)

    @property
    def i2i_active(self):
        return self.use_item_item and self._i2i is not None and self.i2i_alpha > 0.0

    @property
    def has_variants(self):
        """True when a branch outside the fused step is on (BPRLoss then takes the autograd path)."""
        return self.use_pop_gate or self.i2i_active

    def _i2i_apply(self, x, transpose):
        st = self._state()
        key = 'i2i_t' if transpose else 'i2i'
        if key not in st:
            m = self._i2i.T.tocsr() if transpose else self._i2i
            m.sort_indices()
            dev = self._table.device
            st[key] = _lib.Graph(torch.from_numpy(m.indptr.astype(np.int32)).to(dev), torch.from_numpy(m.indices.astype(np.int32)).to(dev),
                                 torch.from_numpy(m.data.astype(np.float32)).to(dev), d_max=self.latent_dim)
        x = x.contiguous().float()
        return x + self.i2i_alpha * st[key].spmm(x, _lib.F32)

    def _fuse_item_embeddings(self, items_emb):
        """model.py:139-157: gate * items + (1 - gate) * pop_vec, gate = sigmoid(gate_mlp([items, pop_vec]) / T)."""
        pop_vec = self.pop_mlp(self.item_pop_scalar.unsqueeze(1))
        gate_logit = self.gate_mlp(torch.cat([items_emb, pop_vec], dim=1))
        if self.pop_gate_temp != 1.0:
            gate_logit = gate_logit / self.pop_gate_temp
        gate = torch.sigmoid(gate_logit)
        self._last_item_gate = gate
        return gate * items_emb + (1.0 - gate) * pop_vec

    def _propagate_dense(self):
        st = self._state()
        N, d, K = self.n_users + self.m_items, self.latent_dim, self.n_layers
        act_dtype = _act_code(self._act())
        work = st.get('eval_work')
        if K > 1 and (work is None or st.get('eval_work_dtype') != act_dtype):
            work = st['eval_work'] = _act_tables(K - 1, N, d, act_dtype, self._table.device)
            st['eval_work_dtype'] = act_dtype
        out = torch.empty(N, d, dtype=torch.float32, device=self._table.device)
        if self.layer_weights is not None:
            w = np.ascontiguousarray(self.layer_weights, dtype=np.float32)
            _lib.check(_lib.load().lgcn_propagate_weighted(
                st['graph'].handle, _lib.tp(self._table), K, d, act_dtype, _lib.tp(work) if K > 1 else None,
                w.ctypes.data_as(C.c_void_p), _lib.tp(out), _lib.current_stream()), "lgcn_propagate_weighted")
            return out
        _lib.check(_lib.load().lgcn_propagate_mean(
            st['graph'].handle, _lib.tp(self._table), K, d, act_dtype, _lib.tp(work) if K > 1 else None,
            _lib.tp(out), _lib.current_stream()), "lgcn_propagate_mean")
        return out

    # -- reference API --------------------------------------------------------------------
    def invalidate_cache(self):
        """Hook probed by main.py:190-191 before each Test."""
        self._cache = None
        self._rating_cache = None
        self._cosine_cache = None

    def train(self, mode=True):
        self.invalidate_cache()
        return super().train(mode)

    def propagated_table(self):
        """The [N,d] fp32 table computer() splits into users / items (item-item smoothing included), memoised
        between invalidate_cache() / train() calls."""
        if self._cache is None:
            with torch.no_grad():
                out = self._propagate_dense()
                cr = getattr(self, 'col_range', None)
                if cr is not None and cr[1] - cr[0] < cr[2]:
                    # a column shard of a wider model (parallel.column_shard): propagation is per column, so the ranks' propagated
                    # columns side by side ARE the full propagated table -- what evaluation has to score with
                    import torch.distributed as dist
                    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() * (cr[1] - cr[0]) == cr[2]):
                        raise _lib.LgcnError("this model holds columns %d..%d of %d: evaluation needs the process group that holds the others" % cr)
                    parts = [torch.empty_like(out) for _ in range(dist.get_world_size())]
                    dist.all_gather(parts, out.contiguous())
                    out = torch.cat(parts, dim=1)
                if self.i2i_active:
                    out = torch.cat([out[:self.n_users], self._i2i_apply(out[self.n_users:], transpose=False)], dim=0)
                self._cache = out
        return self._cache

    def rating_table(self):
        """What getUsersRating scores with (model.py:114-123): the propagated users and the FINAL item
        embeddings (popularity-gated when the gate is on).  This is what the fused evaluation kernels read."""
        if self.score_kind == 'cosine':          # --score cosine: evaluation ranks what was trained, the rows over their norms
            if getattr(self, '_cosine_cache', None) is None:
                with torch.no_grad():
                    self._cosine_cache = _unit_rows(self.propagated_table()).contiguous()
            return self._cosine_cache
        if not self.use_pop_gate:
            return self.propagated_table()
        if getattr(self, '_rating_cache', None) is None:
            with torch.no_grad():
                out = self.propagated_table()
                self._rating_cache = torch.cat([out[:self.n_users], self._fuse_item_embeddings(out[self.n_users:])], dim=0).contiguous()
        return self._rating_cache

    def computer(self):
        """model.py:201-231 -> (all_users [n_users,d], all_items [m_items,d])."""
        if not self.training and not torch.is_grad_enabled():
            out = self.propagated_table()       # eval: propagate once instead of once per user batch
            return out[:self.n_users, :], out[self.n_users:, :]
        if torch.is_grad_enabled() and (self.embedding_user.weight.requires_grad
                                        or self.embedding_item.weight.requires_grad):
            if self.dropout and self.training:
                raise RuntimeError("--dropout 1 is implemented in the fused training step only (BPRLoss.stageOne / fused_step / "
                                   "fused_epoch): the autograd path of computer() / bpr_loss would train without edge dropout")
            out = _Propagate.apply(self.embedding_user.weight, self.embedding_item.weight, self)
        else:
            out = self._propagate_dense()
        all_users, all_items = out[:self.n_users, :], out[self.n_users:, :]
        if self.i2i_active:                      # model.py:228-229
            all_items = _I2ISmooth.apply(all_items, self) if all_items.requires_grad else self._i2i_apply(all_items, False)
        return all_users, all_items

    def getUsersRating(self, users):
        all_users, all_items = self.computer()
        if self.score_kind == 'cosine':          # U^ P^^T: what --loss inbatch --score cosine trains
            return torch.matmul(_unit_rows(all_users[users]), _unit_rows(all_items).t())
        i_emb = self._fuse_item_embeddings(all_items) if self.use_pop_gate else all_items
        return torch.matmul(all_users[users], i_emb.t())

    def getEmbedding(self, users, pos_items, neg_items):
        all_users, all_items = self.computer()
        i_emb = self._fuse_item_embeddings(all_items) if self.use_pop_gate else all_items
        return all_users[users], i_emb[pos_items], i_emb[neg_items], all_users, all_items

    def _bpr_loss_multi(self, users, pos, neg):
        """bpr_loss for R negatives per positive, neg [B, R] (or [R, B]): the autograd statement of the loss of
        lgcn_train_step_multi -- bpr = -mean_{b,r} logsigmoid(x_{b,r}), reg = 0.5/B sum_b (|u|^2 + |p|^2 + 1/R sum_r |n_r|^2)."""
        if self.has_variants:
            raise _lib.LgcnError("several negatives per positive (--neg_ratio > 1) are implemented for the default model, not with "
                                 "--use_pop_gate / --use_item_item")
        B = int(users.shape[0])
        if neg.shape[0] != B:
            neg = neg.t()
        if neg.shape[0] != B:
            raise ValueError(f"neg must be [B, R] or [R, B] with B = {B}, got {tuple(neg.shape)}")
        R = int(neg.shape[1])
        u, pos_e, neg_e, _, _ = self.getEmbedding(users, pos, neg)          # neg_e [B, R, d]
        x = torch.sum(u * pos_e, dim=1)[:, None] - torch.sum(u[:, None, :] * neg_e, dim=2)
        if self.loss_kind == 'softmax':      # l_b = log(1 + sum_r exp(-x_{b,r} / tau)), one term per sample
            z = -x / float(self.softmax_temp)
            bpr = torch.logsumexp(torch.cat([torch.zeros_like(z[:, :1]), z], dim=1), dim=1).sum() / float(B)
        else:
            bpr = -torch.mean(F.logsigmoid(x))
        if self._reg_ego():
            u, pos_e, neg_e = self.embedding_user.weight[users.long()], self.embedding_item.weight[pos.long()], self.embedding_item.weight[neg.long()]
        reg_loss = (0.5 * (u.norm(2).pow(2) + pos_e.norm(2).pow(2) + neg_e.norm(2).pow(2) / float(R))) / float(B)
        return bpr, reg_loss

    def _inbatch_loss(self, users, pos):
        """bpr_loss under --loss inbatch: the autograd statement of the loss of lgcn_train_step_inbatch -- (sm, reg),
        sm = 1/B sum_b logsumexp over {0} and z_{b,c} = (s_{b,c} - s_{b,b}) / tau for c != b, p_c != p_b, u_c != u_b."""
        B = int(users.shape[0])
        all_users, all_items = self.computer()
        ul, pl = users.long(), pos.long()
        u, p = all_users[ul], all_items[pl]
        # --score cosine: the rows over their norms (F.normalize; a row of norm 0 scores 0).  The reg term stays on the rows
        # (eps below every fp32 norm whose square does not underflow: F.normalize then IS e / |e|, and a zero row stays zero)
        s = F.normalize(u, dim=1, eps=1e-37) @ F.normalize(p, dim=1, eps=1e-37).t() if self.score_kind == 'cosine' else u @ p.t()
        z = (s - torch.diagonal(s)[:, None]) / float(self.softmax_temp)
        if self.inbatch_logq:                    # --inbatch_logq 1: z_{b,c} -= lq_{p_c} - lq_{p_b}
            lq = self._item_logq.to(device=z.device, dtype=z.dtype)[pl]
            z = z - (lq[None, :] - lq[:, None])
        keep = (pl[None, :] != pl[:, None]) & (ul[None, :] != ul[:, None])          # (u_c != u_b leaves c = b out too)
        z = torch.where(keep, z, torch.full_like(z, float('-inf')))
        sm = torch.logsumexp(torch.cat([torch.zeros_like(z[:, :1]), z], dim=1), dim=1).sum() / float(B)
        if self._reg_ego():
            u, p = self.embedding_user.weight[ul], self.embedding_item.weight[pl]
        return sm, (0.5 * (u.norm(2).pow(2) + p.norm(2).pow(2))) / float(B)

    def _directau_loss(self, users, pos):
        """bpr_loss under --loss directau: the autograd statement of the loss of lgcn_train_step_directau -- (au, reg),
        au = mean_b |x_b - y_b|^2 + gamma (unif(X) + unif(Y)) / 2, unif(X) = log mean_{b<c} exp(-2 |x_b - x_c|^2) over the pairs by
        position (torch.pdist; 0 for a batch of one), x, y the output rows over their norms."""
        B = int(users.shape[0])
        all_users, all_items = self.computer()
        ul, pl = users.long(), pos.long()
        u, p = all_users[ul], all_items[pl]
        x, y = F.normalize(u, dim=1, eps=1e-37), F.normalize(p, dim=1, eps=1e-37)
        au = (x - y).pow(2).sum() / float(B)
        if B >= 2 and self.au_gamma != 0.0:
            unif = sum(torch.log(torch.exp(-2.0 * torch.pdist(t, p=2).pow(2)).mean()) for t in (x, y))
            au = au + float(self.au_gamma) * unif / 2.0
        if self._reg_ego():
            u, p = self.embedding_user.weight[ul], self.embedding_item.weight[pl]
        return au, (0.5 * (u.norm(2).pow(2) + p.norm(2).pow(2))) / float(B)

    def _inbatch_mix_loss(self, users, pos, neg):
        """bpr_loss under --loss inbatch --inbatch_mix 1: the autograd statement of the loss of lgcn_train_step_inbatch_mix (DESIGN
        4.21) -- logsumexp over the masked [B, 1 + B + B R] logits: the positive's 0, the in-batch columns of _inbatch_loss and the
        pool columns (c, r), masked where n_{c,r} = p_b only.  neg: [B], [B, R] or [R, B]."""
        B = int(users.shape[0])
        neg = torch.as_tensor(neg)
        neg = neg.reshape(B, 1) if neg.dim() == 1 else (neg if neg.shape[0] == B else neg.t())
        if neg.dim() != 2 or neg.shape[0] != B:
            raise ValueError(f"neg must be [B], [B, R] or [R, B] with B = {B}, got {tuple(neg.shape)}")
        R = int(neg.shape[1])
        all_users, all_items = self.computer()
        ul, pl, nl = users.long(), pos.long(), neg.long().to(users.device).t().reshape(-1)      # pool column r B + c = n_{c,r}
        u, p, n = all_users[ul], all_items[pl], all_items[nl]
        cos = self.score_kind == 'cosine'
        uh = F.normalize(u, dim=1, eps=1e-37) if cos else u
        items = torch.cat([p, n], dim=0)
        s = uh @ (F.normalize(items, dim=1, eps=1e-37) if cos else items).t()          # [B, B + B R]
        z = (s - torch.diagonal(s[:, :B])[:, None]) / float(self.softmax_temp)
        if self.inbatch_logq:
            lq = self._item_logq.to(device=z.device, dtype=z.dtype)
            z = z - (torch.cat([lq[pl], lq[nl]])[None, :] - lq[pl][:, None])
        keep = torch.cat([(pl[None, :] != pl[:, None]) & (ul[None, :] != ul[:, None]), nl[None, :] != pl[:, None]], dim=1)
        z = torch.where(keep, z, torch.full_like(z, float('-inf')))
        sm = torch.logsumexp(torch.cat([torch.zeros_like(z[:, :1]), z], dim=1), dim=1).sum() / float(B)
        if self._reg_ego():
            u, p, n = self.embedding_user.weight[ul], self.embedding_item.weight[pl], self.embedding_item.weight[nl]
        return sm, (0.5 * (u.norm(2).pow(2) + p.norm(2).pow(2) + n.norm(2).pow(2) / float(R))) / float(B)

    def hard_neg_select(self, users, neg):
        """--hard_neg M on neg [B, R]: the index r of the candidate each sample trains on -> int64 [B], without gradient.  The
        fused step's selection restated: s_r = e_u.e_{n_r} on the output table, ranked descending with ties by r ascending (a stable
        sort), rank j_b = hard_neg_rank(--seed, step, b, M) picked; step = hard_neg_step, or the Adam step counter as it stands.
        That counter belongs to the fused context: it is 0 while none exists and only fused steps advance it.  A caller that
        trains through autograd with an optimiser of its own must therefore set hard_neg_step to its step count before every
        call (0 before the first) -- otherwise, with M > 1, sample index b draws the same rank j_b in every step."""
        B, R = int(neg.shape[0]), int(neg.shape[1])
        if B != int(users.shape[0]) or R < 2 or self.hard_neg > R:
            raise ValueError(f"--hard_neg {self.hard_neg}: neg must be [B, R] or [R, B] with B = {int(users.shape[0])}, R >= 2 and "
                             f"R >= {self.hard_neg}, got {tuple(neg.shape)}")
        step = self.adam_step if self.hard_neg_step is None else int(self.hard_neg_step)
        j = hard_neg_rank(int(self.config.get('seed', 2020)), step, np.arange(B), self.hard_neg)
        with torch.no_grad():
            all_users, all_items = self.computer()
            s = torch.sum(all_users[users.long()][:, None, :] * all_items[neg.long()], dim=2)
            order = torch.sort(s, dim=1, descending=True, stable=True).indices
            return order.gather(1, torch.from_numpy(j).to(order.device)[:, None]).reshape(-1)

    def last_selection(self):
        """The selected index r of every sample of the last fused step under --hard_neg (-1: a voided sample) -> int32 device
        tensor [max_batch]; its first B entries are the step's.  Needs config['hard_neg_record'] = 1 when the context is made."""
        sel = (self._dev or {}).get('hard_neg_sel')
        if sel is None:
            raise _lib.LgcnError("last_selection: no selection is recorded (--hard_neg with config['hard_neg_record'] = 1, after a fused step)")
        return sel

    def bpr_loss(self, users, pos, neg):
        """model.py:162-183 (unfused, autograd-capable): (bpr [- entropy term of the gate], reg_loss).  Under --hard_neg with 2-D
        negatives the picks are keyed with hard_neg_step, which the caller advances (hard_neg_select says why)."""
        if self.loss_kind == 'inbatch' and self.inbatch_mix:      # the sampled negatives are the batch's shared pool
            return self._inbatch_mix_loss(users, pos, neg)
        if self.loss_kind == 'inbatch':          # the sampled negatives are not used
            return self._inbatch_loss(users, pos)
        if self.loss_kind == 'directau':         # no negatives at all
            return self._directau_loss(users, pos)
        if torch.is_tensor(neg) and neg.dim() == 2 and self.hard_neg:      # the BPR loss of the selected triplets
            neg = neg if neg.shape[0] == int(users.shape[0]) else neg.t()
            sel = self.hard_neg_select(users, neg)
            return self.bpr_loss(users, pos, neg.gather(1, sel[:, None]).reshape(-1))
        if torch.is_tensor(neg) and neg.dim() == 2:
            return self._bpr_loss_multi(users, pos, neg)
        if self.loss_kind == 'softmax':          # 1-D negatives: R = 1
            return self._bpr_loss_multi(users, pos, torch.as_tensor(neg).reshape(-1, 1))
        u, pos_e, neg_e, _, _ = self.getEmbedding(users, pos, neg)
        pos_scores = torch.sum(u * pos_e, dim=1)
        neg_scores = torch.sum(u * neg_e, dim=1)
        bpr = -torch.mean(F.logsigmoid(pos_scores - neg_scores))
        if self._reg_ego():      # upstream LightGCN: userEmb0 / posEmb0 / negEmb0
            u0, p0, n0 = self.embedding_user.weight[users.long()], self.embedding_item.weight[pos.long()], self.embedding_item.weight[neg.long()]
            reg_loss = (0.5 * (u0.norm(2).pow(2) + p0.norm(2).pow(2) + n0.norm(2).pow(2))) / float(u.shape[0])
        else:
            reg_loss = (0.5 * (u.norm(2).pow(2) + pos_e.norm(2).pow(2) + neg_e.norm(2).pow(2))) / float(u.shape[0])
        loss = bpr
        if self.use_pop_gate and hasattr(self, "_last_item_gate"):
            gates = torch.cat([self._last_item_gate[pos], self._last_item_gate[neg]], dim=0)
            gates = torch.clamp(gates, 1e-6, 1.0 - 1e-6)
            entropy = -(gates * torch.log(gates) + (1 - gates) * torch.log(1 - gates)).mean()
            loss = loss - self.gate_entropy_coeff * entropy
        return loss, reg_loss

    def forward(self, users, items):
        all_users, all_items = self.computer()
        i_emb = self._fuse_item_embeddings(all_items) if self.use_pop_gate else all_items
        return (all_users[users] * i_emb[items]).sum(dim=1)

    # -- fused path: which entry point a batch goes to ------------------------------------------
    @staticmethod
    def _neg_dim(neg):
        return neg.dim() if torch.is_tensor(neg) else np.asarray(neg).ndim

    def _negs_rn(self, neg, n, dev, mixed=False):
        """Negatives of n samples -> contiguous int32 [R, n] on the device (negative column r in row r).  Accepts [n, R] (the
        sampler's S[:, 2:]; taken when both readings fit) and [R, n] (Procedure.sample_epoch_to_device).  The multi-negative
        path passes 2-D negatives and gets None for R == 1 unless the loss is softmax (the three-slot step); the mixed
        in-batch path also takes 1-D as R = 1 and holds R to --neg_ratio."""
        neg = self._ids(neg, dev)
        if mixed and neg.dim() == 1:
            neg = neg.reshape(1, -1)
        elif neg.shape[0] == n:
            neg = neg.t()
        if neg.dim() != 2 or neg.shape[1] != n:
            raise ValueError(f"neg must be [{n}], [{n}, R] or [R, {n}], got {tuple(neg.shape)}" if mixed else
                             f"neg must be [{n}, R] or [R, {n}], got {tuple(neg.shape)}")
        R = int(neg.shape[0])
        if mixed:
            if not 1 <= R <= self.neg_ratio:
                raise ValueError(f"--inbatch_mix 1: the batch carries {R} negatives per positive, --neg_ratio is {self.neg_ratio}")
        elif R == 1 and self.loss_kind != 'softmax':
            return None
        elif not 1 <= R <= _lib.MAX_NEG_RATIO:
            raise ValueError(f"the negative ratio (neg_ratio) must be in 1..{_lib.MAX_NEG_RATIO}, got {R} negatives per positive")
        return neg.contiguous()

    def _dispatch(self, users, pos, neg, batch_size=None):
        """_TableModel._dispatch by the loss and the shape of neg: directau and in-batch (neg accepted and ignored), mixed in-batch (neg the
        pool: 1-D, [n, R] or [R, n]), multi-negative ([n, R] or [R, n]; under --loss softmax 1-D too, as R = 1) or three-slot
        (1-D, or one column).  The arguments are each entry point's own (include/lgcn_hip.h)."""
        step = batch_size is None
        if self.has_variants and not self.fused_variants:
            raise RuntimeError("this configuration of the popularity gate / item-item smoothing is outside the fused step "
                               "(--fused_variants 0, or gate hidden sizes > 64 / d > 128): use BPRLoss.stageOne (autograd path)" if step else
                               "this configuration of the optional branches is outside the fused step: loop BPRLoss.stageOne")
        dev = self._table.device
        if self.loss_kind == 'directau':         # neg accepted and ignored
            held = users, pos = self._ids(users, dev).reshape(-1), self._ids(pos, dev).reshape(-1)
            T = int(users.numel())
            u, p = _lib.tp(users), _lib.tp(pos)
            return ("lgcn_train_step_directau", (u, p, T), T, held) if step else ("lgcn_train_epoch_directau", (u, p, T, batch_size), T, held)
        if self.loss_kind == 'inbatch':
            held = users, pos = self._ids(users, dev).reshape(-1), self._ids(pos, dev).reshape(-1)
            T = int(users.numel())
            u, p = _lib.tp(users), _lib.tp(pos)
            if not self.inbatch_mix:
                return ("lgcn_train_step_inbatch", (u, p, T), T, held) if step else ("lgcn_train_epoch_inbatch", (u, p, T, batch_size), T, held)
            negs = self._negs_rn(neg, T, dev, mixed=True)
            n, R, held = _lib.tp(negs), int(negs.shape[0]), (users, pos, negs)
            return ("lgcn_train_step_inbatch_mix", (u, p, n, T, R, T), T, held) if step else ("lgcn_train_epoch_inbatch_mix", (u, p, n, R, T, batch_size), T, held)
        if self.loss_kind == 'softmax' and self._neg_dim(neg) == 1:      # --loss softmax: every shape is a multi step, R = 1 included
            neg = self._ids(neg, dev).reshape(1, -1)
        if self._neg_dim(neg) == 2:            # several negatives per positive: neg [n, R] (the sampler's S[:, 2:]) or [R, n]
            users, pos = self._ids(users, dev), self._ids(pos, dev)
            T = int(users.numel())
            negs = self._negs_rn(neg, T, dev)
            if negs is not None:               # (negative column r at negs + r * T)
                u, p, n, R, held = _lib.tp(users), _lib.tp(pos), _lib.tp(negs), int(negs.shape[0]), (users, pos, negs)
                return ("lgcn_train_step_multi", (u, p, n, T, R, T), T, held) if step else ("lgcn_train_epoch_multi", (u, p, n, R, T, batch_size), T, held)
            neg = self._ids(neg, dev).reshape(-1)     # R == 1: the three-slot form, unchanged
        # the reference's call shape: three torch.long device tensors (main.py:217-225) -- narrowed inside the step's own launch
        # sequence (lgcn_train_step_i64) instead of three conversion kernels and allocations here
        if not (step and all(torch.is_tensor(t) and t.dtype == torch.int64 and t.device == dev and t.is_contiguous() for t in (users, pos, neg))):
            return _TableModel._dispatch(self, users, pos, neg, batch_size)
        B = int(users.numel())
        ids = (_lib.tp(users), _lib.tp(pos), _lib.tp(neg), B)

        def with_scratch(st):
            if st.get('ids32') is None or st['ids32'].numel() < 3 * B:
                st['ids32'] = torch.empty(3 * max(B, st['max_batch']), dtype=torch.int32, device=dev)
            return (*ids, _lib.tp(st['ids32']))
        return "lgcn_train_step_i64", with_scratch, B, (users, pos, neg)


class PureMF(_TableModel):
    """Matrix factorisation trained with BPR: upstream LightGCN's second model (`--model mf`, the class the reference's
    register.py:43-44 registers when it exists) and the baseline every LightGCN number is read against.

    Same constructor `(config, dataset)` and state_dict keys as LightGCN; the tables keep nn.Embedding's own N(0, 1) init
    (upstream PureMF calls no normal_), and live in ONE contiguous [N, d] fp32 table, rows [0, n_users) the users.  No graph
    is built or loaded.  BPRLoss.stageOne / fused_step / fused_epoch run the two HIP launches of csrc/lgcn_mf.hip
    (lgcn_mf_train_step / _epoch: loss, gradient rows, dense torch.optim.Adam); there is no CPU fallback.  `bpr_loss` is the
    plain torch restatement on the parameter views (autograd-capable: what the fused step is cross-checked against).

    `--layer` is ignored.  The fork's optional branches and the LightGCN-only switches are refused at construction."""
    has_variants = False
    fused_variants = False
    use_pop_gate = False
    dropout = False
    layer_weights = None
    _CTX = {'destroy': 'lgcn_mf_destroy', 'get_step': 'lgcn_mf_get_step', 'set_step': 'lgcn_mf_set_step', 'set_lr': 'lgcn_mf_set_lr',
            'check': 'lgcn_mf_check', 'step': 'lgcn_mf_train_step', 'epoch': 'lgcn_mf_train_epoch'}

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        no = "is not implemented for --model mf"
        if config.get('use_pop_gate', False):
            raise _lib.LgcnError(f"--use_pop_gate {no} (the popularity gate belongs to LightGCN)")
        if config.get('use_item_item', False):
            raise _lib.LgcnError(f"--use_item_item {no} (the item-item smoothing belongs to LightGCN)")
        if int(config.get('dropout', 0)):
            raise _lib.LgcnError(f"--dropout 1 {no} (there is no graph whose edges could be dropped)")
        lw = config.get('layer_weights', 'mean')
        if not (lw is None or (isinstance(lw, str) and lw.strip().lower() == 'mean')):
            raise _lib.LgcnError(f"--layer_weights {lw} {no} (there are no layers to combine)")
        if config.get('use_ppr_weights', False):
            raise _lib.LgcnError(f"--use_ppr_weights {no} (there are no layers to combine)")
        if self._act() != 'fp32':
            raise _lib.LgcnError(f"--act_dtype {config.get('act_dtype')} {no} (fp32 tables only)")
        if int(config.get('hard_neg', 0)) != 0:      # (before --neg_ratio, which it implies)
            raise _lib.LgcnError(f"--hard_neg {config.get('hard_neg')} {no} (hard negatives are picked among LightGCN's --neg_ratio candidates)")
        if int(config.get('neg_ratio', 1)) != 1:
            raise _lib.LgcnError(f"--neg_ratio {config.get('neg_ratio')} {no} (the matrix-factorisation step trains on triplets, "
                                 "one negative per positive)")
        if str(config.get('loss', 'bpr')).strip().lower() != 'bpr':
            raise _lib.LgcnError(f"--loss {config.get('loss')} {no} (the matrix-factorisation step computes the BPR loss)")
        if str(config.get('score', 'dot')).strip().lower() != 'dot':
            raise _lib.LgcnError(f"--score {config.get('score')} {no} (an option of LightGCN's --loss inbatch)")
        if str(config.get('inbatch_logq', 0)).strip().lower() not in ('0', 'false'):
            raise _lib.LgcnError(f"--inbatch_logq {config.get('inbatch_logq')} {no} (an option of LightGCN's --loss inbatch)")
        if str(config.get('inbatch_mix', 0)).strip().lower() not in ('0', 'false'):
            raise _lib.LgcnError(f"--inbatch_mix {config.get('inbatch_mix')} {no} (an option of LightGCN's --loss inbatch)")
        if self.latent_dim not in (32, 64, 128, 256):
            raise ValueError("latent_dim_rec must be 32, 64, 128 or 256 for the HIP kernels")
        if self.n_users + self.m_items >= 2 ** 31:
            raise ValueError("n_users + m_items must stay below 2^31")
        # RNG consumption of upstream PureMF: the two nn.Embedding constructors in this order, their own N(0, 1) init kept
        self.embedding_user = nn.Embedding(self.n_users, self.latent_dim)
        self.embedding_item = nn.Embedding(self.m_items, self.latent_dim)
        self._bind_table()
        self.f = nn.Sigmoid()

    # -- device state: the context of csrc/lgcn_mf.hip over the table, Adam's moments and a step's workspace ----
    def _ctx_stale(self, st, dp_world, rows):
        return st.get('table_ptr') != self._table.data_ptr()

    def _make_ctx(self, max_batch, dp_world=1, rows=None):
        st = self._dev
        old_step = self._retire_ctx(st)
        self._step_workspace(st, 2 * max_batch)
        cfg = self._fill_step_config(_lib.MfConfig(), st, max_batch)
        cfg.m_items = self.m_items
        st['ctx'] = self._create_ctx('lgcn_mf_create', cfg, [('lgcn_mf_set_step', (old_step,))])
        st['max_batch'], st['table_ptr'] = max_batch, self._table.data_ptr()

    # -- reference API --------------------------------------------------------------------
    def propagated_table(self):
        """The [N, d] fp32 table computer() splits into users / items: the parameters themselves."""
        return self._table

    def rating_table(self):
        """What the fused evaluation kernels rank with: the table itself, i.e. the RAW scores U . I^T.  getUsersRating applies
        a sigmoid, which is monotone and in fp32 merges distinct scores (everything above ~16.6 becomes 1.0), so ranking the
        raw scores refines upstream's ranking and never contradicts it."""
        return self._table

    def computer(self):
        """-> (all_users [n_users, d], all_items [m_items, d]): the two parameter views."""
        return self.embedding_user.weight, self.embedding_item.weight

    def getUsersRating(self, users):
        all_users, all_items = self.computer()
        return self.f(torch.matmul(all_users[users.long()], all_items.t()))

    def getEmbedding(self, users, pos_items, neg_items):
        all_users, all_items = self.computer()
        return all_users[users.long()], all_items[pos_items.long()], all_items[neg_items.long()], all_users, all_items

    def bpr_loss(self, users, pos, neg):
        """Upstream PureMF.bpr_loss in plain torch (autograd-capable): (mean softplus(neg - pos), reg_loss)."""
        u, pos_e, neg_e, _, _ = self.getEmbedding(users, pos, neg)
        pos_scores = torch.sum(u * pos_e, dim=1)
        neg_scores = torch.sum(u * neg_e, dim=1)
        loss = torch.mean(F.softplus(neg_scores - pos_scores))
        reg_loss = (0.5 * (u.norm(2).pow(2) + pos_e.norm(2).pow(2) + neg_e.norm(2).pow(2))) / float(u.shape[0])
        return loss, reg_loss

    def forward(self, users, items):
        all_users, all_items = self.computer()
        return self.f(torch.sum(all_users[users.long()] * all_items[items.long()], dim=1))
