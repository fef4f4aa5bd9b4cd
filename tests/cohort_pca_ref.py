"""The cohort PCA of include/oai_hip.h ("Cohort PCA") restated in numpy, operation for operation: the whitening, the ordered dot (a chunk
loop, and inside it a loop over vertices), the ordered combine, and the whole fit and transform of stats.ThicknessPCA.  The device
(csrc/cohort_pca.hip) must equal this file to the bit; tests/test_cohort_pca_cpu.py holds this file to np.linalg.svd and sklearn."""
from types import SimpleNamespace

import numpy as np

CHUNK = 512                # vertices per chunk of the ordered dot
DROP = 1e-12               # a component is kept where lambda > 0 and lambda > DROP * lambda_1


def valid_entries(Y, mask):
    """bool [N, V]: the mask is non-zero (None: everywhere) and the value is not NaN."""
    ok = ~np.isnan(Y)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def counted_mean(Y, mask):
    """(mean float64 [V], n [V]) as oai_group_prepare forms them: the valid values summed in ascending knee index with one accumulator,
    divided by their count; NaN where there is none."""
    ok = valid_entries(Y, mask)
    total = np.zeros(Y.shape[1])
    for i in range(Y.shape[0]):
        total = total + np.where(ok[i], Y[i].astype(np.float64), 0.0)
    n = ok.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return total / n.astype(np.float64), n


def whiten(Y, mask, mean, rw):
    """a_iv = ((double) y_iv - mean_v) * rw_v, one subtraction then one product; exactly 0.0 by a select where the entry is missing or
    rw_v == 0."""
    ok = valid_entries(Y, mask) & (rw != 0.0)[None, :]
    with np.errstate(invalid="ignore"):
        centred = Y.astype(np.float64) - mean[None, :]
        return np.where(ok, centred * rw[None, :], 0.0)


def ordered_dot(A, B):
    """C_ij = sum_v a_iv b_jv: chunks of 512 vertices; inside a chunk ascending v into one accumulator from 0.0, a product then an add;
    the chunk sums in ascending chunk index into one accumulator from 0.0."""
    V = A.shape[1]
    total = np.zeros((A.shape[0], B.shape[0]))
    for c0 in range(0, V, CHUNK):
        acc = np.zeros_like(total)
        for v in range(c0, min(c0 + CHUNK, V)):
            acc = acc + A[:, v, None] * B[None, :, v]
        total = total + acc
    return total


def norm2(A):
    """sum_v a_iv^2 in the ordered-dot order: the diagonal of ordered_dot(A, A)."""
    V = A.shape[1]
    total = np.zeros(A.shape[0])
    for c0 in range(0, V, CHUNK):
        acc = np.zeros_like(total)
        for v in range(c0, min(c0 + CHUNK, V)):
            acc = acc + A[:, v] * A[:, v]
        total = total + acc
    return total


def combine(coef, rows):
    """R_cv = sum_i k_ci a_iv over ascending i into one accumulator, a product then an add."""
    out = np.zeros((coef.shape[0], rows.shape[1]))
    for i in range(rows.shape[0]):
        out = out + coef[:, i, None] * rows[None, i, :]
    return out


def eigen(G, n_components):
    """(lambda [K], U [N, K], s [K]) of the Gram matrix: np.linalg.eigh, descending; kept where lambda > 0 and lambda > 1e-12 lambda_1;
    K = min(n_components, kept)."""
    lam, U = np.linalg.eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    kept = int(((lam > 0.0) & (lam > DROP * lam[0])).sum())
    K = min(int(n_components), kept)
    if K < 1:
        raise ValueError("the cohort has no variance: every whitened knee is zero")
    lam, U = lam[:K].copy(), np.ascontiguousarray(U[:, :K])
    return lam, U, np.sqrt(lam)


def sign_modes(R, U):
    """Each mode signed so that its entry of largest |value| is positive, the lowest vertex winning ties; the knees' coordinates follow."""
    R, U = R.copy(), U.copy()
    for c in range(R.shape[0]):
        if R[c, int(np.argmax(np.abs(R[c])))] < 0.0:
            R[c], U[:, c] = -R[c], -U[:, c]
    return R, U


def root_weights(weights, n, min_valid):
    """(rw [V], n_excluded): np.sqrt of the weights, 0 where fewer than min_valid knees have a value."""
    out = n < min_valid
    return np.where(out, 0.0, np.sqrt(np.asarray(weights, np.float64))), int(out.sum())


def fit(Y, mask, weights, n_components=10, min_valid=2):
    """ThicknessPCA.fit on host arrays: float32 Y [N, V], a mask or None, float64 weights [V] (areas in mm^2, or ones)."""
    N = Y.shape[0]
    mean, n = counted_mean(Y, mask)
    rw, n_excluded = root_weights(weights, n, min_valid)
    A = whiten(Y, mask, mean, rw)
    G = ordered_dot(A, A)
    lam, U, s = eigen(G, n_components)
    R = combine(np.ascontiguousarray(U.T / s[:, None]), A)
    R, U = sign_modes(R, U)
    with np.errstate(invalid="ignore", divide="ignore"):
        modes_mm = np.where(rw[None, :] != 0.0, R / rw[None, :], np.nan)
    return SimpleNamespace(mean=mean, n=n, rw=rw, n_excluded=n_excluded, A=A, G=G, modes_w=R, modes_mm=modes_mm, singular_values=s,
                           explained_variance=lam / (N - 1), explained_variance_ratio=lam / G.diagonal().sum(), scores=s[None, :] * U)


def score_record(scores, norm2_rows, explained_variance):
    """(t2, q, q_fraction) of knees with these scores and squared whitened norms."""
    inside = (scores * scores).sum(axis=1)
    q = norm2_rows - inside
    with np.errstate(invalid="ignore", divide="ignore"):
        return (scores * scores / explained_variance[None, :]).sum(axis=1), q, q / norm2_rows


def transform(model, Y, mask):
    """ThicknessPCA.transform on host arrays: the knees whitened with the model's mean and root weights, scores = ordered_dot(A', R)."""
    A = whiten(Y, mask, model.mean, model.rw)
    scores = ordered_dot(A, model.modes_w)
    t2, q, q_fraction = score_record(scores, norm2(A), model.explained_variance)
    n_missing = (~valid_entries(Y, mask) & (model.rw != 0.0)[None, :]).sum(axis=1)
    return SimpleNamespace(scores=scores, t2=t2, q=q, q_fraction=q_fraction, n_missing=n_missing)
