"""Float64 yardstick of NIQE (Mittal, Soundararajan, Bovik 2013) as BasicSR's ``calculate_niqe`` computes it, numpy only, one
function per pass.  PARITY UNPINNED: BasicSR, OpenCV and ``niqe_pris_params.npz`` are not at hand; the formulas are BasicSR's,
restated (tests/test_host_niqe.py holds a direct transcription on scipy and checks this file against it).

1. ``plane``      8-bit codes ``rint(clamp(x, 0, 1) 255)`` (one fp32 multiply, as the luma kernels form them), ``shave`` pixels
                  cut from each border, ``Y = round_half_even(16 + (65481 r + 128553 g + 24966 b) / 255000)`` in integers,
                  cropped at the bottom and right to multiples of 96.
2. ``mscn``       ``mu = w (*) x``, ``sigma = sqrt(|w (*) x^2 - mu^2|)``, ``v = (x - mu) / (sigma + 1)`` with the 7 x 7 window
                  convolved over replicated borders (scipy's ``convolve(mode='nearest')``): one multiply and one add per tap,
                  each rounded, in row-major window order from 0.  Scale 2 runs on ``half_plane``, the bicubic antialiased
                  x0.5 of the plane in its 0..255 scale (BasicSR resizes img / 255 and multiplies back: the operator is linear,
                  the two differ by rounding only).
3. ``moments``    per block (96 at scale 1, 48 at scale 2; row-major grid) and map ``v``, ``v roll(v, (0, 1))``, ``v roll(v,
                  (1, 0))``, ``v roll(v, (1, 1))``, ``v roll(v, (1, -1))`` -- ``np.roll`` inside the block -- the five numbers
                  ``count(< 0), count(> 0), sum_{<0} m^2, sum_{>0} m^2, sum |m|``.
4. ``fit``        the AGGD fit from those numbers; ``features_from_moments`` strings 10 fits into the 36 features of a block.
5. ``statistics`` / ``score``.

On a flat neighbourhood x - mu is rounding residue and so is the sign of v; BasicSR has the same property.  ``min_local_variance``
and ``unstable_fits`` let a test assert that its inputs stay clear of that and of alpha's grid steps."""
import math
import warnings

import numpy as np

import imresize_ref

BLOCK = 96
GRID = np.arange(0.2, 10.001, 0.001)
assert GRID.shape == (9801,)
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def gaussian_window(size=7, sigma=7.0 / 6.0):
    """MATLAB's fspecial('gaussian', 7, 7/6): exp(-(x^2 + y^2) / (2 sigma^2)) over -3..3, divided by its sum."""
    r = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


# ----------------------------------------------------------------------------- 1. the plane
def codes(x):
    """int64 8-bit codes of a float array, formed in fp32 like the device: rint(clamp(x, 0, 1) * 255.0f)."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int64)


def plane(x, shave=0):
    """[N, 3, H, W] floats -> float64 [N, Hc, Wc] integer lumas."""
    c = codes(x)
    n, ch, h, w = c.shape
    assert ch == 3
    if shave:
        c = c[:, :, shave:h - shave, shave:w - shave]
    t = 65481 * c[:, 0] + 128553 * c[:, 1] + 24966 * c[:, 2]
    q, rem = np.divmod(t, 255000)
    q = q + ((rem > 127500) | ((rem == 127500) & (q % 2 == 1)))
    y = 16 + q
    nby, nbx = max(y.shape[1], 0) // BLOCK, max(y.shape[2], 0) // BLOCK
    if nby * nbx < 2:
        raise ValueError("fewer than two 96 x 96 blocks")
    return y[:, :nby * BLOCK, :nbx * BLOCK].astype(np.float64)


def luma_ties():
    """[((r, g, b), q)] with 65481 r + 128553 g + 24966 b = 255000 q + 127500: one of each parity of q."""
    out = {}
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for r in range(256):
        t = 65481 * r + 128553 * g + 24966 * b
        hit = np.argwhere(t % 255000 == 127500)
        for gi, bi in hit:
            q = int(t[gi, bi] // 255000)
            out.setdefault(q % 2, ((r, int(gi), int(bi)), q))
        if len(out) == 2:
            break
    return [out[k] for k in sorted(out)]


def half_plane(p):
    """The scale-2 input in float64: MATLAB-style bicubic antialiased imresize by 0.5 of the 0..255 plane."""
    return imresize_ref.resize(p, scale=0.5)


# ----------------------------------------------------------------------------- 2. MSCN
def _window_sums(x, window):
    h, w = x.shape[-2:]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(3, 3), (3, 3)], mode="edge")
    mu = np.zeros_like(x)
    ex2 = np.zeros_like(x)
    for a in range(7):
        for b in range(7):                       # convolution: window element (a, b) meets the pixel at (i + 3 - a, j + 3 - b)
            s = xp[..., 6 - a:6 - a + h, 6 - b:6 - b + w]
            mu = mu + window[a, b] * s
            ex2 = ex2 + window[a, b] * (s * s)
    return mu, ex2


def mscn(x, window=None):
    x = np.asarray(x, dtype=np.float64)
    window = gaussian_window() if window is None else np.asarray(window, dtype=np.float64)
    mu, ex2 = _window_sums(x, window)
    return (x - mu) / (np.sqrt(np.abs(ex2 - mu * mu)) + 1.0)


def min_local_variance(p, window=None, region=None):
    """The smallest |w (*) x^2 - mu^2| over a plane, or over its part ``[..., region[0], region[1]]`` (two slices): what
    ``v``'s relative error is divided by."""
    x = np.asarray(p, dtype=np.float64)
    window = gaussian_window() if window is None else np.asarray(window, dtype=np.float64)
    mu, ex2 = _window_sums(x, window)
    var = np.abs(ex2 - mu * mu)
    if region is not None:
        var = var[..., region[0], region[1]]
    return float(var.min())


# ----------------------------------------------------------------------------- 3. moments
def block_maps(blk):
    return [blk] + [blk * np.roll(blk, s, axis=(0, 1)) for s in SHIFTS]


def moments(v, block):
    """float64 [..., nb, 5, 5] of an MSCN image [..., h, w] whose sides are multiples of `block`."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim > 2:
        return np.stack([moments(p, block) for p in v])
    nby, nbx = v.shape[0] // block, v.shape[1] // block
    out = np.zeros((nby * nbx, 5, 5), dtype=np.float64)
    for by in range(nby):
        for bx in range(nbx):
            blk = v[by * block:(by + 1) * block, bx * block:(bx + 1) * block]
            for k, m in enumerate(block_maps(blk)):
                neg, pos = m < 0, m > 0
                out[by * nbx + bx, k] = (neg.sum(), pos.sum(), (m[neg] ** 2).sum(), (m[pos] ** 2).sum(), np.abs(m).sum())
    return out


# ----------------------------------------------------------------------------- 4. the fit
_TABLES = None


def gamma_tables():
    """(r, bscale, mscale) over GRID: Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)), sqrt(Gamma(1/a) / Gamma(3/a)), Gamma(2/a) /
    Gamma(1/a), float64 from math.gamma."""
    global _TABLES
    if _TABLES is None:
        g1 = np.array([math.gamma(1.0 / a) for a in GRID])
        g2 = np.array([math.gamma(2.0 / a) for a in GRID])
        g3 = np.array([math.gamma(3.0 / a) for a in GRID])
        _TABLES = (g2 * g2 / (g1 * g3), np.sqrt(g1 / g3), g2 / g1)
    return _TABLES


def r_norm(m, block):
    """r_hat_n of one map's five numbers (NaN when a side is empty)."""
    nneg, npos, sneg, spos, sabs = (float(t) for t in m)
    b2 = float(block * block)
    with np.errstate(all="ignore"):
        ls = np.sqrt(np.float64(sneg) / np.float64(nneg))
        rs = np.sqrt(np.float64(spos) / np.float64(npos))
        gh = ls / rs
        rhat = (np.float64(sabs) / b2) ** 2 / ((np.float64(sneg) + np.float64(spos)) / b2)
        rn = rhat * (gh ** 3 + 1.0) * (gh + 1.0) / ((gh ** 2 + 1.0) ** 2)
    return float(rn), float(ls), float(rs)


def alpha_index(rn):
    r = gamma_tables()[0]
    with np.errstate(all="ignore"):
        return int(np.argmin((r - rn) ** 2))           # all-NaN: 0


def fit(m, block):
    """(index, alpha, beta_l, beta_r, mean factor) of one map."""
    rn, ls, rs = r_norm(m, block)
    i = alpha_index(rn)
    _, bscale, mscale = gamma_tables()
    return i, float(GRID[i]), ls * bscale[i], rs * bscale[i], mscale[i]


def features_from_moments(m1, m2):
    """(features float64 [nb, 36], alpha indices int [nb, 10]) from the moments [nb, 5, 5] of scale 1 and scale 2."""
    nb = m1.shape[0]
    feat = np.zeros((nb, 36), dtype=np.float64)
    idx = np.zeros((nb, 10), dtype=np.int64)
    for b in range(nb):
        row = []
        for s, (m, block) in enumerate(((m1, BLOCK), (m2, BLOCK // 2))):
            for k in range(5):
                i, alpha, bl, br, ms = fit(m[b, k], block)
                idx[b, s * 5 + k] = i
                row += [alpha, (bl + br) / 2.0] if k == 0 else [alpha, (br - bl) * ms, bl, br]
        feat[b] = row
    return feat, idx


def unstable_fits(moment_pair, rel):
    """[(scale, block, map)] of the fits whose alpha index changes when r_hat_n moves by a factor 1 +- rel."""
    out = []
    for s, (m, block) in enumerate(zip(moment_pair, (BLOCK, BLOCK // 2))):
        m = np.asarray(m).reshape(-1, 5, 5)
        for b in range(m.shape[0]):
            for k in range(5):
                rn = r_norm(m[b, k], block)[0]
                if math.isnan(rn):
                    continue
                if len({alpha_index(rn * (1.0 - rel)), alpha_index(rn), alpha_index(rn * (1.0 + rel))}) != 1:
                    out.append((s, b, k))
    return out


def image_moments(p, window=None, p2=None):
    """(m1, m2) of one plane [Hc, Wc]; `p2` replaces the float64 half-size plane (e.g. by the device's fp32 one)."""
    p2 = half_plane(p) if p2 is None else np.asarray(p2, dtype=np.float64)
    return moments(mscn(p, window), BLOCK), moments(mscn(p2, window), BLOCK // 2)


def features(x, shave=0, window=None):
    """float64 [N, nb, 36] of [N, 3, H, W] floats: steps 1 to 4."""
    return np.stack([features_from_moments(*image_moments(p, window))[0] for p in plane(x, shave)])


# ----------------------------------------------------------------------------- 5. statistics and score
def statistics(feat):
    """(mu_d [36], cov_d [36, 36], NaN-free row count) of one image's [nb, 36] table; cov_d is NaN below two rows."""
    feat = np.asarray(feat, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mu = np.nanmean(feat, axis=0)
    good = feat[~np.isnan(feat).any(axis=1)]
    cov = np.cov(good, rowvar=False) if good.shape[0] >= 2 else np.full((36, 36), np.nan)
    return mu, cov, int(good.shape[0])


def score(mu_p, cov_p, mu_d, cov_d, count):
    if count < 2 or np.isnan(mu_d).any():
        return float("nan")
    d = (np.asarray(mu_p, dtype=np.float64).reshape(1, 36) - mu_d.reshape(1, 36))
    inv = np.linalg.pinv((np.asarray(cov_p, dtype=np.float64) + cov_d) / 2.0)
    return float(np.sqrt(d @ inv @ d.T).item())


def niqe(x, mu_p, cov_p, shave=0, window=None):
    """float64 [N]: the score of each image of [N, 3, H, W]."""
    return np.array([score(mu_p, cov_p, *statistics(f)) for f in features(x, shave, window)])
