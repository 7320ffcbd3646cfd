"""Restatements of the CTC head's kernels (kernels/ctc.h) for the tests, and their inputs:
    ctc_reference(logits, target)      numpy fp64: -log p(target | log_softmax(logits)) and its gradient by alpha-beta
    greedy(logits)                     the greedy CTC rule -> (path, length, conf) as ccd_ctc_greedy lays them out
    torch_oracle(logits, targets, dt)  F.ctc_loss(F.log_softmax(logits.to(dt), -1), ..., reduction='none', zero_infinity=True) on the
                                       CPU with autograd down to the logits (the issue's oracle)
    named_cases() / random_batch()     the inputs of tests/test_ctc_{sim,gpu}.py
"""
import numpy as np
import torch
import torch.nn.functional as F

NEG = -np.inf


def _lse(values):
    m = max(values)
    if m == NEG:
        return NEG
    return m + np.log(sum(np.exp(v - m) for v in values))


def ctc_reference(logits, target):
    """logits [T, C] -> (nll or inf, d nll / d logits [T, C]; zeros when infeasible), fp64."""
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    logp = x - np.array([_lse(list(row)) for row in x])[:, None]
    ext = [0]
    for c in target:
        ext += [int(c), 0]
    S = len(ext)
    alpha = np.full((T, S), NEG)
    beta = np.full((T, S), NEG)
    alpha[0, 0] = logp[0, 0]
    if S > 1:
        alpha[0, 1] = logp[0, ext[1]]
    for t in range(1, T):
        for s in range(S):
            terms = [alpha[t - 1, s]]
            if s >= 1:
                terms.append(alpha[t - 1, s - 1])
            if s >= 2 and ext[s] != 0 and ext[s] != ext[s - 2]:
                terms.append(alpha[t - 1, s - 2])
            alpha[t, s] = _lse(terms) + logp[t, ext[s]]
    ll = _lse([alpha[T - 1, S - 1]] + ([alpha[T - 1, S - 2]] if S > 1 else []))
    if ll == NEG:
        return np.inf, np.zeros_like(x)
    beta[T - 1, S - 1] = logp[T - 1, ext[S - 1]]
    if S > 1:
        beta[T - 1, S - 2] = logp[T - 1, ext[S - 2]]
    for t in range(T - 2, -1, -1):
        for s in range(S):
            terms = [beta[t + 1, s]]
            if s + 1 < S:
                terms.append(beta[t + 1, s + 1])
            if s + 2 < S and ext[s + 2] != 0 and ext[s + 2] != ext[s]:
                terms.append(beta[t + 1, s + 2])
            beta[t, s] = _lse(terms) + logp[t, ext[s]]
    grad = np.exp(logp)
    for t in range(T):
        for c in set(ext):
            tot = _lse([alpha[t, s] + beta[t, s] for s in range(S) if ext[s] == c])
            if tot > NEG:
                grad[t, c] -= np.exp(tot - logp[t, c] - ll)
    return -ll, grad


def greedy(logits):
    """logits [B, T, C] -> path int32 [B, T] (-1-padded), length int32 [B], conf fp32 [B, T] (0-padded)."""
    x = np.asarray(logits, dtype=np.float32)
    B, T, _ = x.shape
    path, conf = np.full((B, T), -1, np.int32), np.zeros((B, T), np.float32)
    length = np.zeros(B, np.int32)
    for b in range(B):
        before = -1
        for t in range(T):
            c = int(np.argmax(x[b, t]))                                  # numpy: the first maximum
            if c != 0 and c != before:
                e = np.exp(x[b, t].astype(np.float64) - np.float64(x[b, t, c]))
                path[b, length[b]], conf[b, length[b]] = c, 1.0 / e.sum()
                length[b] += 1
            before = c
    return path, length, conf


def label_lengths(targets):
    """int64 [B, Lmax] zero-padded -> the count of leading non-zero entries."""
    t = np.asarray(targets)
    return np.where((t == 0).any(1), (t == 0).argmax(1), t.shape[1]) if t.shape[1] else np.zeros(len(t), np.int64)


def torch_oracle(logits, targets, dtype):
    """logits [B, T, C] (tensor), targets int64 [B, Lmax] zero-padded -> (per-sample loss with inf kept [B], nll with zero_infinity [B],
    gradient of sum_b nll_b / max(L_b, 1) / B down to the logits [B, T, C]) in `dtype`, on the CPU."""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    t = targets.cpu().long()
    B, T, _ = x.shape
    L = torch.from_numpy(label_lengths(t.numpy())).long()
    flat = torch.cat([t[b, :L[b]] for b in range(B)]) if B else t.flatten()
    lp = F.log_softmax(x, -1).transpose(0, 1)                               # [T, B, C]
    frames = torch.full((B,), T, dtype=torch.long)
    raw = F.ctc_loss(lp, flat, frames, L, blank=0, reduction="none", zero_infinity=False)
    nll = F.ctc_loss(lp, flat, frames, L, blank=0, reduction="none", zero_infinity=True)
    (nll / L.clamp_min(1).to(dtype) / B).sum().backward()
    return raw.detach(), nll.detach(), x.grad.detach()


def _case(name, T, C, target, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return dict(name=name, T=T, C=C, target=list(target), logits=torch.randn(T, C, generator=g) * scale)


def named_cases():
    """The named cases of the loss kernel (T = 32, C = 92 unless stated); feasibility is torch's verdict, asserted in the checks."""
    distinct = list(range(1, 26))
    rep7 = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7] + list(range(8, 19))               # L = 25, 7 adjacent repeats: 32 frames
    rep8 = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8] + list(range(9, 18))          # L = 25, 8 adjacent repeats: 33 frames
    alt31 = [1 + (i & 1) for i in range(31)]
    cases = [
        _case("01_L0", 32, 92, [], 101),
        _case("02_L1", 32, 92, [17], 102),
        _case("03_aa", 32, 92, [11, 11], 103),
        _case("04_16_equal", 32, 92, [5] * 16, 104),                                       # needs 31 frames
        _case("05_17_equal", 32, 92, [5] * 17, 105),                                       # needs 33 frames
        _case("06_L25_distinct", 32, 92, distinct, 106),
        _case("07_L25_7_repeats", 32, 92, rep7, 107),
        _case("08_L25_8_repeats", 32, 92, rep8, 108),
        _case("09_L31_alternating", 32, 92, alt31, 109),
        _case("10_L31_one_repeat", 32, 92, alt31[:15] + [alt31[14]] + alt31[15:30], 110),  # 31 + 1 = 32 frames: torch aligns it
        _case("10b_L31_two_repeats", 32, 92, [3, 3] + alt31[:14] + [alt31[13]] + alt31[14:28], 1110),    # 33 frames
        _case("11_logits_x80", 32, 92, [9, 30, 30, 4, 61, 9], 111, scale=80.0),
        _case("12_C128_label127", 32, 128, [127, 1, 127, 127, 64], 112),
        _case("13_C3", 32, 3, [1, 2, 2, 1], 113),
        _case("14_T1_L0", 1, 92, [], 114),
        _case("14_T1_L1", 1, 92, [40], 115),
        _case("15_T64_L31", 64, 92, alt31, 116),
    ]
    assert all(len(c["target"]) <= 31 for c in cases) and len(cases[9]["target"]) == len(cases[10]["target"]) == 31
    return cases


def random_batch(B, seed, T=32, C=92, Lmax=25, max_len=16):
    """B samples with L <= 16 (always feasible at T = 32: L + repeats <= 2 L - 1), a small alphabet so that characters repeat."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, C, generator=g) * 2.0
    targets = torch.zeros(B, Lmax, dtype=torch.long)
    for b in range(B):
        L = int(torch.randint(0, max_len + 1, (1,), generator=g))
        hi = 6 if b % 2 else C                                              # every other sample: labels from 1..5
        targets[b, :L] = torch.randint(1, hi, (L,), generator=g)
    return logits, targets


def pad_targets(target, Lmax=31):
    row = torch.zeros(1, Lmax, dtype=torch.long)
    row[0, :len(target)] = torch.tensor(target, dtype=torch.long)
    return row
