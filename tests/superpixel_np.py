"""Float64 restatement of Dino/metric/eval_superpixel.py for the tests (torch fp64 on the CPU, autograd-capable), the loader of
tests/golden/superpixel_cases.npz and the seeded inputs the kernel tests use.

The window is applied as two zero-padded 1-D correlations with the fp32 taps of `gaussian(ws, 1.5)` taken as exact fp64 numbers;
the statistics are E[x y] - E[x] E[y] as in the metric's definition, all in fp64."""
import os

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps64(ws):
    from ccd_amd.metric.eval_superpixel import gaussian
    return gaussian(ws, 1.5).double()


def blur(x, ws):
    """Zero-padded separable Gaussian correlation of every plane of x [N, C, H, W] (fp64), same size."""
    g = taps64(ws).to(x.device)
    r = ws // 2
    N, C, H, W = x.shape
    p = x.reshape(N * C, 1, H, W)
    p = F.conv2d(p, g.view(1, 1, 1, ws), padding=(0, r))
    p = F.conv2d(p, g.view(1, 1, ws, 1), padding=(r, 0))
    return p.reshape(N, C, H, W)


def ssim_map(imgs, ws):
    """The SSIM (2 images) or TRI_SSIM (3 images) map, fp64 [N, C, H, W]."""
    xs = [x.double() for x in imgs]
    mu = [blur(x, ws) for x in xs]
    var = [blur(x * x, ws) - m * m for x, m in zip(xs, mu)]
    pairs = [(0, 1)] if len(xs) == 2 else [(0, 1), (1, 2), (2, 0)]
    cov = [blur(xs[i] * xs[j], ws) - mu[i] * mu[j] for i, j in pairs]
    k = 2.0 if len(xs) == 2 else 1.0
    num = (k * sum(mu[i] * mu[j] for i, j in pairs) + C1) * (k * sum(cov) + C2)
    den = (sum(m * m for m in mu) + C1) * (sum(var) + C2)
    return num / den


def ssim(imgs, ws, size_average=True):
    m = ssim_map(imgs, ws)
    return m.mean() if size_average else m.flatten(1).mean(1)


def psnr(a, b):
    """-> (psnr fp64 0-dim or inf, mse fp64) over the first three channels."""
    d = a[:, :3].double() * 255.0 - b[:, :3].double() * 255.0
    mse = (d * d).mean()
    if mse.item() == 0:
        return float("inf"), mse
    return 20.0 * torch.log10(255.0 / torch.sqrt(mse)), mse


def grads(fn, imgs):
    """fp64 autograd gradients of fn(list of fp64 leaves) w.r.t. every image."""
    leaves = [x.detach().double().requires_grad_(True) for x in imgs]
    fn(leaves).backward()
    return [x.grad for x in leaves]


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------ inputs
def uniform(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32)


def text_like(n, c, h, w, seed):
    """ccd_amd.synthetic text-like views rescaled to [0, 1] per image (flat background, strokes), [n, c, h, w] fp32."""
    from ccd_amd.synthetic import make_text_like_batch
    img, _, _ = make_text_like_batch((n + 2) // 3, seed=seed)
    img = img.float().reshape(-1, 3, 32, 128)[:n]             # the three views of each sample are images of their own
    if tuple(img.shape[2:]) != (h, w):
        img = F.interpolate(img, size=(h, w), mode="bilinear", align_corners=False)
    if img.shape[1] < c:
        img = torch.cat([img, img[:, :c - img.shape[1]]], 1)
    img = img[:, :c]
    lo = img.flatten(1).min(1).values.view(-1, 1, 1, 1)
    hi = img.flatten(1).max(1).values.view(-1, 1, 1, 1)
    return ((img - lo) / (hi - lo).clamp_min(1e-12)).contiguous()


def perturbed(x, seed, amp=0.08):
    """x plus seeded noise, clipped to [0, 1] (a 'super-resolved' version of x)."""
    g = torch.Generator().manual_seed(seed)
    return (x + amp * torch.randn(x.shape, generator=g, dtype=torch.float32)).clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------ fixtures
def load_cases(golden_dir):
    """-> (case names, {name: {key: np.ndarray}}, {window size: (gaussian taps, create_window(ws, 3))})."""
    z = np.load(os.path.join(golden_dir, "superpixel_cases.npz"))
    names = [str(n) for n in z["names"]]
    cases = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}
    windows = {int(w): (z[f"gaussian/{int(w)}"], z[f"window/{int(w)}"]) for w in z["window_sizes"]}
    return names, cases, windows
