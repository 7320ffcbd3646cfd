"""The text super-resolution task restated in numpy (fp64): the specification the kernels of kernels/sr.h are checked against.

    bicubic_x2(lr)      F.interpolate(lr, scale_factor=2, mode="bicubic", align_corners=False): A = -0.75, border indices clamped
    gradient_map(x)     g = sqrt((0.5 (x[y, x+1] - x[y, x-1]))^2 + (0.5 (x[y-1, x] - x[y+1, x]))^2 + 1e-6), zero padding (TSRN)
    sr_loss(sr, hr)     L = mean_n (mse_n + gp_weight gp_n), mse_n = mean (sr - hr)^2, gp_n = mean |g(sr) - g(hr)| over 3 H W;
                        its gradient with sign(0) = 0, scaled by d_loss
"""
import numpy as np

GP_EPS = 1e-6
A = -0.75


def cubic_taps(t):
    """The four weights of the cubic convolution kernel at fraction t (torch's get_cubic_upsample_coefficients)."""
    def near(x):
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def far(x):
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.array([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)])


def _axis_x2(x, axis):
    n = x.shape[axis]
    o = np.arange(2 * n)
    src = (o + 0.5) / 2.0 - 0.5
    f = np.floor(src).astype(np.int64)
    t = src - f
    out = 0.0
    for k in range(4):
        w = np.array([cubic_taps(tt)[k] for tt in t])
        shape = [1] * x.ndim
        shape[axis] = 2 * n
        out = out + np.take(x, np.clip(f - 1 + k, 0, n - 1), axis=axis) * w.reshape(shape)
    return out


def bicubic_x2(lr):
    """[..., h, w] -> [..., 2h, 2w] in fp64, not clamped."""
    return _axis_x2(_axis_x2(np.asarray(lr, np.float64), -1), -2)


def normalise(base, mean, std):
    return (base - np.asarray(mean, np.float64)[:, None, None]) / np.asarray(std, np.float64)[:, None, None]


def _halved_differences(x):
    p = np.pad(np.asarray(x, np.float64), [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)])
    a = 0.5 * (p[..., 1:-1, 2:] - p[..., 1:-1, :-2])
    b = 0.5 * (p[..., :-2, 1:-1] - p[..., 2:, 1:-1])
    return a, b


def gradient_map(x):
    a, b = _halved_differences(x)
    return np.sqrt(a * a + b * b + GP_EPS)


def sign_margin(sr, hr):
    """min |g(sr) - g(hr)| over all pixels: the sign of the gradient-profile term must not hang on a rounding."""
    return float(np.abs(gradient_map(sr) - gradient_map(hr)).min())


def gp_backward(sr, hr):
    """d/d sr of sum |g(sr) - g(hr)| as a gather: pixel q collects from the four pixels whose stencil contains it."""
    a, b = _halved_differences(sr)
    g = np.sqrt(a * a + b * b + GP_EPS)
    s = np.sign(g - gradient_map(hr))
    ca = np.pad(0.5 * s * a / g, [(0, 0)] * (sr.ndim - 2) + [(1, 1), (1, 1)])      # what p gives to p + ex (and minus that to p - ex)
    cb = np.pad(0.5 * s * b / g, [(0, 0)] * (sr.ndim - 2) + [(1, 1), (1, 1)])      # what p gives to p - ey (and minus that to p + ey)
    return ca[..., 1:-1, :-2] - ca[..., 1:-1, 2:] + cb[..., 2:, 1:-1] - cb[..., :-2, 1:-1]


def gp_backward_brute(sr, hr):
    """The same by a double loop over one plane [H, W]: every pixel p scatters into its four stencil points."""
    sr, hr = np.asarray(sr, np.float64), np.asarray(hr, np.float64)
    H, W = sr.shape
    at = lambda x, y, xx: x[y, xx] if 0 <= y < H and 0 <= xx < W else 0.0
    out = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            g = []
            for img in (sr, hr):
                a = 0.5 * (at(img, y, x + 1) - at(img, y, x - 1))
                b = 0.5 * (at(img, y - 1, x) - at(img, y + 1, x))
                g.append((a, b, np.sqrt(a * a + b * b + GP_EPS)))
            (a, b, gs), s = g[0], np.sign(g[0][2] - g[1][2])
            for (yy, xx), d in (((y, x + 1), 0.5 * a), ((y, x - 1), -0.5 * a), ((y - 1, x), 0.5 * b), ((y + 1, x), -0.5 * b)):
                if 0 <= yy < H and 0 <= xx < W:
                    out[yy, xx] += s * d / gs
    return out


def sr_loss(sr, hr, gp_weight=1e-4, d_loss=1.0):
    """sr, hr [N, 3, H, W] -> dict(loss, parts [L, mean mse, mean gp], mse [N], gp [N], grad [N, 3, H, W])."""
    sr, hr = np.asarray(sr, np.float64), np.asarray(hr, np.float64)
    N = sr.shape[0]
    if N == 0:
        return dict(loss=0.0, parts=np.zeros(3), mse=np.zeros(0), gp=np.zeros(0), grad=np.zeros(sr.shape))
    mse = ((sr - hr) ** 2).reshape(N, -1).mean(axis=1)
    gp = np.abs(gradient_map(sr) - gradient_map(hr)).reshape(N, -1).mean(axis=1)
    loss = float((mse + gp_weight * gp).mean())
    per = sr[0].size * N
    grad = d_loss * (2.0 * (sr - hr) + gp_weight * gp_backward(sr, hr)) / per
    return dict(loss=loss, parts=np.array([loss, mse.mean(), gp.mean()]), mse=mse, gp=gp, grad=grad)
