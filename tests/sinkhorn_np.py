"""numpy restatements of DINOLoss.sinkhorn_knopp_teacher (Dino/loss/Dino_loss.py:157-184), in our own words, and the helpers the
Sinkhorn tests share.

linear(t, temp, n)      the reference's loop as written: Q = exp(t / temp)^T, scaled to total 1, then n rounds of "every prototype
                        gets 1/K, every sample gets 1/B", and the final * B.  dtype float64 by default; float32 shows what fp32 costs
                        the reference's formulation (and where it stops being finite).
potentials(t, temp, n)  the same iteration on logarithms: log beta_k = -logsumexp_r(x + log alpha_r), log alpha_r =
                        -logsumexp_k(x + log beta_k); n column steps, n - 1 row steps.  Returns c = -temp * log beta, mean 0.
assignment(t, c, temp)  softmax_k((t - c) / temp): equals linear(t, temp, n) because the reference's last step normalises every
                        sample, and its constants (K, B, sum_Q) are common factors of a row.
"""
import os

import numpy as np

FIXTURE = "sinkhorn_cases.npz"
FLOOR = 1e-12          # probabilities below it are compared absolutely only (atol of every gate)


def linear(t, temp, n_iterations=3, dtype=np.float64):
    t = np.asarray(t, dtype=dtype)
    q = np.exp(t / dtype(temp)).T                       # [K, B]
    k, b = q.shape
    q = q / q.sum()
    for _ in range(n_iterations):
        q = q / q.sum(axis=1, keepdims=True)
        q = q / dtype(k)
        q = q / q.sum(axis=0, keepdims=True)
        q = q / dtype(b)
    return (q * dtype(b)).T


def _lse(v, axis):
    m = v.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def potentials(t, temp, n_iterations=3):
    x = np.asarray(t, dtype=np.float64) / float(temp)
    log_alpha = np.zeros(x.shape[0])
    for it in range(n_iterations):
        log_beta = -_lse(x + log_alpha[:, None], 0)
        if it + 1 < n_iterations:
            log_alpha = -_lse(x + log_beta[None, :], 1)
    c = -float(temp) * log_beta
    return c - c.mean()


def assignment(t, c, temp):
    v = (np.asarray(t, dtype=np.float64) - np.asarray(c, dtype=np.float64)[None, :]) / float(temp)
    v = v - v.max(axis=1, keepdims=True)
    e = np.exp(v)
    return e / e.sum(axis=1, keepdims=True)


def restatement(t, temp, n_iterations=3):
    """float64 assignment through the log domain: finite for every finite input."""
    return assignment(t, potentials(t, temp, n_iterations), temp)


def deviation(got, want):
    """Largest relative deviation over the entries of `want` at or above FLOOR (inf where `got` is not finite)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    live = want >= FLOOR
    return float((np.abs(got - want)[live] / want[live]).max()) if live.any() else 0.0


def cosine_logits(rows, k, seed, dim=32):
    """Clamped cosine products, entries in [-1, 1]: what the weight-normed last layer hands the loss."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((rows, dim))
    w = g.standard_normal((k, dim))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    return np.clip(2.5 * (a @ w.T), -1.0, 1.0).astype(np.float32)


def format_rtol(t, temp):
    """Gate of the cases that have no recorded reference noise.  One fp32 rounding of a logit-sized quantity moves an entry's
    exponent by 2^-24 * |t - c| / temp, with |t - c| up to the spread of the logits - the reference pays for one such rounding
    (t / temp), we pay for the same and for c.  The fixtures' gate is 4 x the reference's recorded noise; where no noise can be
    recorded (other shapes, inputs at which the fp32 reference overflows) the same factor applies to this bound of one rounding."""
    t = np.asarray(t, dtype=np.float64)
    spread = max(float(t.max() - t.min()), 1.0)
    return 4.0 * 2.0 ** -24 * spread / float(temp)


def load_cases(golden_dir):
    """[(name, dict(t, temp, n, ref, f64, noise))] of tests/golden/sinkhorn_cases.npz."""
    g = np.load(os.path.join(golden_dir, FIXTURE))
    out = []
    for name in [str(n) for n in g["names"]]:
        out.append((name, dict(t=g[name + "/t"], temp=float(g[name + "/temp"]), n=int(g[name + "/n"]), ref=g[name + "/ref"],
                               f64=g[name + "/f64"], noise=float(g[name + "/noise"]))))
    return out


def dino_loss_np(s_logits, q, student_temp=0.1):
    """The distillation term of Dino_loss.py:81-102 from [2M, K] student logits and the [2M, K] teacher assignment q: view 0's
    targets meet view 1's student rows and the other way round."""
    s = np.asarray(s_logits, dtype=np.float64) / student_temp
    s = s - s.max(axis=1, keepdims=True)
    logp = s - np.log(np.exp(s).sum(axis=1, keepdims=True))
    m = len(s) // 2
    q = np.asarray(q, dtype=np.float64)
    terms = [(-q[:m] * logp[m:]).sum(axis=1).mean(), (-q[m:] * logp[:m]).sum(axis=1).mean()]
    return 0.5 * (terms[0] + terms[1])
