"""fp64 torch restatement of the four training-loss terms (closed forms of
include/dstd_gcn_loss.h), for tests that need a reference on inputs the
fixture does not hold.  tests/test_loss_host.py pins it to the reference's own
values and autograd gradients (tests/golden/losses.npz) at 1e-12.

With d = pred - targ per joint, weights w (ones when None), wbar = mean(w):
  jl2 = wbar * mean(w_j ||d||)
  tl2 = wbar * mean over the T-1 frame differences of w_j ||d_{s+1} - d_s||
  cl1 = cl2 = mean(w_j |d_c|)
Gradients come from autograd on these forms: 0 where a norm is 0 and
sign(0) = 0 -- for cl2 that is the project's deliberate deviation from the
reference's NaN at w_j * d_c == 0.
"""
import torch

TERMS = ("jl2", "tl2", "cl1", "cl2")


def loss_terms(pred, targ, w=None):
    """{term: 0-d fp64 tensor} for pred, targ [n][t][V*3] (any float dtype;
    computed in fp64) and w [V] or None.  tl2 is absent when t < 2."""
    pred, targ = pred.double(), torch.as_tensor(targ).double()
    n, t, vc = pred.shape
    V = vc // 3
    w = torch.ones(V, dtype=torch.float64) if w is None else torch.as_tensor(w).double()
    d = (pred - targ).view(n, t, V, 3)
    out = {"jl2": w.mean() * (w * torch.linalg.vector_norm(d, dim=-1)).mean()}
    if t >= 2:
        out["tl2"] = w.mean() * (w * torch.linalg.vector_norm(d[:, 1:] - d[:, :-1], dim=-1)).mean()
    out["cl1"] = (w[:, None] * d.abs()).mean()
    out["cl2"] = (w[:, None] * d.abs()).mean()
    return out


def loss_terms_and_grads(pred, targ, w=None):
    """({term: float}, {term: fp64 gradient w.r.t. pred})."""
    values, grads = {}, {}
    for term in TERMS:
        p = pred.detach().double().requires_grad_(True)
        terms = loss_terms(p, targ, w)
        if term not in terms:
            continue
        terms[term].backward()
        values[term], grads[term] = float(terms[term].detach()), p.grad
    return values, grads
