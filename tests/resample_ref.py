'''The three resampling rules of fd_latent_upscale_noise_f32 (include/flexdiffuse_hip.h) restated in float64 numpy, for
upscaling only: nearest by its integer rule, and the antialiased bilinear / bicubic filters of torch's
interpolate(..., antialias=True) -- separable taps, align_corners = False, taps off the axis dropped, the rest normalised.'''
import numpy as np

MODES = {'nearest': 0, 'bilinear': 1, 'bicubic': 2}
# (hs, ws) -> (H, W): dropped border taps, non-integer ratios, the identity, a one-cell axis
SHAPES = [((5, 7), (8, 13)), ((8, 8), (16, 16)), ((8, 8), (8, 8)), ((3, 4), (9, 5)), ((1, 2), (4, 7))]


def triangle(t):
    t = abs(t)
    return 1.0 - t if t < 1.0 else 0.0


def keys_cubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def nearest_index(i: int, n_in: int, n_out: int) -> int:
    return ((2 * i + 1) * n_in) // (2 * n_out)


def axis_matrix(mode: str, n_in: int, n_out: int) -> np.ndarray:
    '''[n_out][n_in] float64: row i holds the weights of output index i over the source axis.'''
    assert n_out >= n_in >= 1, 'upscaling only'
    m = np.zeros((n_out, n_in), np.float64)
    if mode == 'nearest':
        for i in range(n_out):
            m[i, nearest_index(i, n_in, n_out)] = 1.0
        return m
    f, S = (triangle, 1.0) if mode == 'bilinear' else (keys_cubic, 2.0)
    scale = n_in / n_out
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - S + 0.5)), min(n_in, int(c + S + 0.5))
        w = np.array([f(j - c + 0.5) for j in range(lo, hi)], np.float64)
        m[i, lo:hi] = w / w.sum()
    return m


def resample(src: np.ndarray, H: int, W: int, mode: str) -> np.ndarray:
    '''src (..., hs, ws) -> (..., H, W), float64.'''
    src = np.asarray(src, np.float64)
    return np.einsum('yj,...jk,xk->...yx', axis_matrix(mode, src.shape[-2], H), src, axis_matrix(mode, src.shape[-1], W))


def source(B: int, C: int, hs: int, ws: int, seed: int = 0) -> np.ndarray:
    '''The fp32 source latents the tests share: unit normals from a seeded generator.'''
    return np.random.default_rng(1000 * seed + 10 * hs + ws).standard_normal((B, C, hs, ws)).astype(np.float32)
