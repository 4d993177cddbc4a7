"""Plain torch / scipy restatement of ONE training step with the fork's optional branches -- the popularity gate and the
item-item smoothing (model.py's computer() / _fuse_item_embeddings / bpr_loss): test infrastructure for
tests/test_gate_restatement.py (which pins it to the fixtures recorded from the reference) and tests/test_gpu_gate_shapes.py
(which compares the fused HIP step with it).  It imports nothing from the package.

    X_0 = E,  X_k = A_hat X_{k-1},  T = (X_0 + ... + X_K) / (K + 1)            users = T[:n_users], items = T[n_users:]
    items <- items + (alpha I2I) items                                          (smoothing, when a matrix is given)
    a = relu(W1 s + b1), pv = W2 a + b2, h = relu(V1 [items ; pv] + c1), g = sigmoid((V2 h + c2) / temp)
    F = g items + (1 - g) pv                                                    (gate, when the MLP tensors are given)
    bpr = mean softplus(-(<u, F_p> - <u, F_n>)),  reg = (|u|^2 + |F_p|^2 + |F_n|^2) / (2 B)
    loss = bpr - coeff * mean over the 2B slots of H(clamp(g, 1e-6, 1 - 1e-6)),  total = loss + decay * reg

Everything runs in `dtype`: float64 is the reference, float32 -- the same code, the "fp32 twin" -- measures what rounding alone
does to each quantity and is the yardstick of the tolerances.  Inputs are taken as given (fp32 arrays are widened exactly)."""
import numpy as np
import scipy.sparse as sp
import torch

MLP_NAMES = ("pop_mlp.0.weight", "pop_mlp.0.bias", "pop_mlp.2.weight", "pop_mlp.2.bias",
             "gate_mlp.0.weight", "gate_mlp.0.bias", "gate_mlp.2.weight", "gate_mlp.2.bias")       # named_parameters order
CLAMP = 1e-6
B1, B2, EPS = 0.9, 0.999, 1e-8


def norm_adj(n_users, m_items, users, items):
    """A_hat = D^-1/2 [[0, R], [R^T, 0]] D^-1/2 of the interaction lists, values in fp32 as the dataset object keeps them."""
    r = sp.csr_matrix((np.ones(len(users), np.float32), (users, items)), shape=(n_users, m_items))
    r.data[:] = 1.0                                                   # (a repeated pair counts once)
    a = sp.bmat([[None, r], [r.T, None]]).tocsr().astype(np.float32)
    rowsum = np.asarray(a.sum(axis=1)).ravel().astype(np.float32)
    d_inv = np.zeros_like(rowsum)
    d_inv[rowsum != 0] = np.power(rowsum[rowsum != 0], np.float32(-0.5))
    a = sp.diags(d_inv).dot(a).dot(sp.diags(d_inv)).tocsr().astype(np.float32)
    a.sort_indices()
    return a


def pop_scalar(item_counts):
    """The gate's popularity input: standardised log1p of the items' train counts, in fp32 as the model computes it."""
    pop = torch.log1p(torch.clamp(torch.from_numpy(np.asarray(item_counts, np.float64)).float(), min=0.0))
    return ((pop - pop.mean()) / (pop.std() + 1e-8)).numpy()


def _sparse(m, dtype):
    m = sp.coo_matrix(m)
    ij = torch.from_numpy(np.vstack([m.row, m.col]).astype(np.int64))
    return torch.sparse_coo_tensor(ij, torch.from_numpy(m.data.astype(np.float64)).to(dtype), m.shape).coalesce()


def _bf16_ste(x):
    """Round to bf16 (round to nearest even, torch's cast) with the identity as derivative: a stored activation table."""
    return x + (x.detach().to(torch.bfloat16).to(x.dtype) - x.detach())


def step(adj, table, mlp, pop, i2i, n_users, K, decay, temp, coeff, batch, dtype=torch.float64, act_bf16=False):
    """One loss / gradient evaluation.
    adj: A_hat, scipy sparse [N, N];  table: [N, d];  mlp: the eight MLP tensors in MLP_NAMES order, or None (no gate);
    pop: [m_items] popularity scalar (with mlp);  i2i: alpha * I2I, scipy sparse [m_items, m_items], or None (no smoothing);
    batch: (users, pos, neg) integer arrays;  act_bf16: bf16 activation storage as the fused step has it with a branch on -- all
    K propagated layers are stored in bf16 and, for K >= 2, layer 1 gathers the table rounded to bf16; the layer mean takes the
    table itself.
    -> dict of float64 numpy values: loss (bpr - coeff * entropy), reg, total, bpr, entropy, grad_table [N, d], grad_final [N, d]
       (d total / d T: the gradient rows before the propagation's backward), grad_mlp [8], pre_pop [2B, Hp] and pre_gate
       [2B, Hg] (hidden pre-activations on the batch's item slots, positives first), gates [2B], grad_mlp_abs [8] (for every
       element of every MLP gradient the sum over the 2B slots of |that slot's term|)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)             # (small matrices: a pool as wide as the machine only waits for itself; restored below)
    try:
        return _step(adj, table, mlp, pop, i2i, n_users, K, decay, temp, coeff, batch, dtype, act_bf16)
    finally:
        torch.set_num_threads(threads)


def _step(adj, table, mlp, pop, i2i, n_users, K, decay, temp, coeff, batch, dtype, act_bf16):
    u, p, n = (torch.from_numpy(np.asarray(t).astype(np.int64)) for t in batch)
    E = torch.from_numpy(np.asarray(table, np.float64)).to(dtype).requires_grad_(True)
    A = _sparse(adj, dtype)
    x, acc = (_bf16_ste(E) if act_bf16 and K >= 2 else E), E        # (bf16 storage, K >= 2: layer 1 gathers the bf16 copy of the table)
    for _ in range(K):
        x = torch.sparse.mm(A, x)
        if act_bf16:
            x = _bf16_ste(x)
        acc = acc + x
    T = acc / float(K + 1)
    T.retain_grad()
    users, items = T[:n_users], T[n_users:]
    if i2i is not None:
        items = items + torch.sparse.mm(_sparse(i2i, dtype), items)
    out = {}
    slots = torch.cat([p, n])
    nb = len(p)
    if mlp is not None:
        # the gate on the 2B item slots of the batch (bpr_loss reads nothing else of it), a slot at a time: an item named twice is
        # two slots, so every parameter gradient is a sum of 2B per-slot terms
        W1, b1, W2, b2, V1, c1, V2, c2 = (torch.from_numpy(np.asarray(t, np.float64)).to(dtype).requires_grad_(True) for t in mlp)
        prm = [W1, b1, W2, b2, V1, c1, V2, c2]
        it = items[slots]
        s = torch.from_numpy(np.asarray(pop, np.float64)).to(dtype)[slots][:, None]
        pre_pop = s @ W1.t() + b1
        act = torch.relu(pre_pop)
        pv = act @ W2.t() + b2
        x_in = torch.cat([it, pv], dim=1)
        pre_gate = x_in @ V1.t() + c1
        hid = torch.relu(pre_gate)
        raw_logit = hid @ V2.t() + c2
        logit = raw_logit / temp if temp != 1.0 else raw_logit
        g = torch.sigmoid(logit)
        final = g * it + (1.0 - g) * pv
        for t in (pre_pop, pv, pre_gate, raw_logit):
            t.retain_grad()
        out["pre_pop"], out["pre_gate"], out["gates"] = pre_pop, pre_gate, g[:, 0]
        pe, ne = final[:nb], final[nb:]
    else:
        prm = []
        pe, ne = items[p], items[n]
    ue = users[u]
    bpr = -torch.nn.functional.logsigmoid((ue * pe).sum(1) - (ue * ne).sum(1)).mean()
    reg = 0.5 * (ue.pow(2).sum() + pe.pow(2).sum() + ne.pow(2).sum()) / float(len(u))
    loss = bpr
    if mlp is not None:
        gc = torch.clamp(g, CLAMP, 1.0 - CLAMP)
        ent = -(gc * torch.log(gc) + (1.0 - gc) * torch.log(1.0 - gc)).mean()
        loss = bpr - coeff * ent
        out["entropy"] = ent
    total = loss + decay * reg
    total.backward()
    out.update(loss=loss, reg=reg, total=total, bpr=bpr, grad_table=E.grad, grad_final=T.grad,
               grad_mlp=[t.grad if t.grad is not None else torch.zeros_like(t) for t in prm])
    if mlp is not None:
        # sum over the slots of |per-slot term| for every element of every MLP gradient (weight: |d pre|^T |input|, bias: sum |d pre|)
        pairs = ((pre_pop, s), (pv, act), (pre_gate, x_in), (raw_logit, hid))
        out["grad_mlp_abs"] = [t for dpre, inp_ in pairs for t in (dpre.grad.abs().t() @ inp_.detach().abs(), dpre.grad.abs().sum(0))]
    return {k: ([t.detach().double().numpy() for t in v] if isinstance(v, list) else
                (v.detach().double().numpy() if v.dim() else float(v.detach().double()))) for k, v in out.items()}


def adam(p, m, v, g, step_no, lr, beta1=B1, beta2=B2, eps=EPS):
    """torch.optim.Adam's single-tensor step in float64 (exp_avg.lerp_(g, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2);
    denom = sqrt(v) / sqrt(bc2) + eps; p -= lr / bc1 * m / denom) -> (p', m', v').  step_no counts from 1."""
    p, m, v, g = (np.asarray(t, np.float64) for t in (p, m, v, g))
    m2 = m + (1.0 - beta1) * (g - m)
    v2 = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step_no, 1.0 - beta2 ** step_no
    return p - (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)), m2, v2


def rel_max(got, ref):
    """max |got - ref| as a fraction of max |ref| (0 / 0 = 0): how the distance of a gradient tensor is measured."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = float(np.abs(ref).max()) if ref.size else 0.0
    num = float(np.abs(got - ref).max()) if ref.size else 0.0
    return num / den if den > 0.0 else (0.0 if num == 0.0 else float("inf"))
