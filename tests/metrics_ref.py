"""Float64 statements of the distribution metrics (transformer_latent_diffusion_amd/metrics.py, csrc/tld_metrics.hip): the bank
append, the moments, the pair sum of k - 1, both MMD^2 estimators, the textbook Frechet distance, the tile plan of the pair kernel, and the derived
error bound of the pair sum.  numpy only (scipy for the textbook matrix square root)."""
import numpy as np

TILE, KCHUNK, MAX_DIM = 128, 32, 4096          # FEAT_TILE, FEAT_KCHUNK, FEAT_MAX_DIM (csrc/tld_feat_plan.h)
U32 = 2.0 ** -24                               # unit roundoff of fp32
C_MFMA = 1.5e-7                                # fp32 MFMA chain against fp64 at K <= 1024, relative to |a||b| (the kernel guide's measured figure)


def pitch(dim):
    return (dim + KCHUNK - 1) // KCHUNK * KCHUNK


# ---- the bank ---------------------------------------------------------------------------------------------------------------------------------
def append_ref(x, normalize=True):
    """x [rows, dim] as float32 (a bf16 / fp16 input converted exactly) -> (stored fp32 rows [rows, pitch(dim)], bad row count).  The squares are
    exact in double and added in ascending column order; the quotient is formed in double and rounded to fp32 once."""
    x = np.asarray(x, dtype=np.float32)
    rows, dim = x.shape
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        sq = np.cumsum(x64 * x64, axis=1)[:, -1]                     # cumsum adds in ascending order
        bad = ~np.isfinite(sq) | ((sq == 0.0) if normalize else False)
        val = (x64 / np.sqrt(sq)[:, None]).astype(np.float32) if normalize else x.copy()
    val[bad] = 0.0
    out = np.zeros((rows, pitch(dim)), dtype=np.float32)
    out[:, :dim] = val
    return out, int(bad.sum())


def moments_ref(feats):
    f = np.asarray(feats, dtype=np.float64)
    return f.mean(axis=0), np.atleast_2d(np.cov(f, rowvar=False))


# ---- pair sums and MMD^2 ----------------------------------------------------------------------------------------------------------------------
def sq_dists(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):                                         # from the differences themselves, never from a Gram matrix
        d = b - a[i]
        out[i] = np.einsum("jk,jk->j", d, d)
    return out


def kernel_sum_ref(a, b, gamma, same):
    """sum_ij expm1(-gamma |a_i - b_j|^2); same: b is a and the terms i == j are the constant 0, whatever the subtraction gave."""
    t = np.expm1(-gamma * sq_dists(a, b))
    if same:
        t[np.eye(len(a), dtype=bool)] = 0.0
    return float(np.sum(t))


def mmd2_ref(x, y, sigma=10.0, unbiased=False):
    n, m, g = len(x), len(y), 1.0 / (2.0 * sigma * sigma)
    sxx, syy, sxy = kernel_sum_ref(x, x, g, True), kernel_sum_ref(y, y, g, True), kernel_sum_ref(x, y, g, False)
    dx, dy = (n * (n - 1), m * (m - 1)) if unbiased else (n * n, m * m)
    return sxx / dx + syy / dy - 2.0 * sxy / (n * m)


def pair_bound(a, b, gamma):
    """Bound on |kernel sum - statement| / (number of pairs) for the fp32 arithmetic of tld_feat_kernel_sum on rows a, b (derived, not fitted):
    per pair |delta (k - 1)| <= gamma (4 c |a_i||b_j| + 3 u d2_max) + 2 u |k - 1|_max.  4 c: the dot product twice plus the two norms, each an
    fp32 chain with relative error c; 3 u d2_max: the three roundings that form d2; 2 u |k - 1|: the rounding of the argument and expm1f's.
    |d expm1(-x) / dx| <= 1 turns an error of gamma d2 into one of k - 1.  A mean over pairs keeps the per-pair bound; mmd2 is four such means."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.sqrt((a * a).sum(1)).max(), np.sqrt((b * b).sum(1)).max()
    d2max = sq_dists(a, b).max()
    return gamma * (4.0 * C_MFMA * na * nb + 3.0 * U32 * d2max) + 2.0 * U32 * abs(np.expm1(-gamma * d2max))


# ---- the Frechet distance, textbook form ------------------------------------------------------------------------------------------------------
def frechet_sqrtm(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) with scipy.linalg.sqrtm, the form FID scripts use."""
    from scipy import linalg
    root = linalg.sqrtm(s1 @ s2)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(root).real)


def frechet_inputs(E, n, seed):
    """Two sets of unit rows of randn(n, E) @ randn(E, E), the second shifted before it is normalised."""
    rng = np.random.default_rng(seed)
    out = []
    for shift in (0.0, 0.5):
        x = rng.standard_normal((n, E)) @ rng.standard_normal((E, E)) + shift * np.sqrt(E) * rng.standard_normal(E)
        out.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    return out


# ---- the tile plan ----------------------------------------------------------------------------------------------------------------------------
def tile_plan(na, nb, same):
    """[(ti, tj, weight)] in the order of feat_plan (csrc/tld_feat_plan.h)."""
    if na < 1 or nb < 1 or (same and na != nb):
        return []
    ta, tb = -(-na // TILE), -(-nb // TILE)
    if not same:
        return [(i, j, 1) for i in range(ta) for j in range(tb)]
    return [(i, j, 1 if i == j else 2) for i in range(ta) for j in range(i, ta)]
