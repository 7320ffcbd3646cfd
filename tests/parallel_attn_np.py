"""The parallel attention recognition head in numpy (fp64): the specification of kernels/posattn.h and of
ccd_amd/decoder/parallel_attn_decoder.py.  It is the reference's `Attention.forward` (Dino/modules/attention.py:5-30) followed by
`BaseVision.cls`; tests/golden/parallel_attn.npz (tools/gen_parallel_attn_golden.py) ties it to the reference itself.

Per image n: X = tokens[n] [256, E] (token s = row * 32 + col), T positions, C classes.

    Q0[s, e] = b0[s] + sum_t W0[s, t] F[t, e]            (image-independent)
    P        = X Wv^T + bv
    M        = tanh(P + Q0)
    A[s, t]  = be[t] + sum_e M[s, e] We[t, e]
    a[t, s]  = softmax over the 256 tokens s of A[s, t]
    G[t, e]  = sum_s a[t, s] X[s, e]
    logits   = G Wc^T + bc
"""
import numpy as np

TOKENS = 256


def q0(F, W0, b0):
    return np.asarray(b0, np.float64)[:, None] + np.asarray(W0, np.float64) @ np.asarray(F, np.float64)


def core_forward(P, X, Q0, We, be):
    """What ccd_posattn_fwd computes from its operands: P, X [N, 256, E], Q0 [256, E], We [T, E], be [T] -> (a [N, T, 256], G [N, T, E])."""
    P, X, Q0, We, be = (np.asarray(v, np.float64) for v in (P, X, Q0, We, be))
    M = np.tanh(P + Q0[None])
    A = M @ We.T + be[None, None]                                      # [N, 256, T]
    A = A - A.max(axis=1, keepdims=True)
    e = np.exp(A)
    a = (e / e.sum(axis=1, keepdims=True)).transpose(0, 2, 1)          # [N, T, 256]
    return a, a @ X


def core_backward(dG, X, P, Q0, We, a):
    """The backward formulas given dG [N, T, E]: -> dict(dX1, dP [N, 256, E], dQ0 [256, E], dWe [T, E], dbe [T])."""
    dG, X, P, Q0, We, a = (np.asarray(v, np.float64) for v in (dG, X, P, Q0, We, a))
    M = np.tanh(P + Q0[None])
    da = dG @ X.transpose(0, 2, 1)                                     # [N, T, 256]
    dX1 = a.transpose(0, 2, 1) @ dG
    dA = (a * (da - (a * da).sum(axis=2, keepdims=True))).transpose(0, 2, 1)     # [N, 256, T]
    dM = dA @ We
    dP = dM * (1.0 - M * M)
    return dict(dX1=dX1, dP=dP, dQ0=dP.sum(axis=0), dWe=np.einsum("nst,nse->te", dA, M), dbe=dA.sum(axis=(0, 1)))


def forward(X, w):
    """The whole head: X [N, 256, E], w = dict(F, W0, b0, Wv, bv, We, be[, Wc, bc]) -> dict(Q0, P, a, G[, logits])."""
    X = np.asarray(X, np.float64)
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    Q0 = q0(w["F"], w["W0"], w["b0"])
    P = X @ w["Wv"].T + w["bv"]
    a, G = core_forward(P, X, Q0, w["We"], w["be"])
    out = dict(Q0=Q0, P=P, a=a, G=G)
    if "Wc" in w:
        out["logits"] = G @ w["Wc"].T + w["bc"]
    return out


def backward(dG, X, w):
    """Gradients of every parameter of the attention and of X under dG [N, T, E] (the formulas of the issue, in fp64)."""
    X = np.asarray(X, np.float64)
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    f = forward(X, w)
    g = core_backward(dG, X, f["P"], f["Q0"], w["We"], f["a"])
    dP, dQ0 = g["dP"], g["dQ0"]
    return dict(dF=w["W0"].T @ dQ0, dW0=dQ0 @ w["F"].T, db0=dQ0.sum(axis=1), dWv=np.einsum("nso,nsi->oi", dP, X), dbv=dP.sum(axis=(0, 1)),
                dWe=g["dWe"], dbe=g["dbe"], dX=g["dX1"] + dP @ w["Wv"])
