"""frog_modes (include/frog_chain.h) restated in NumPy: one rounded float64 operation per stated line, on the stored planes.
`planes` is (n_images, nz, ny, nx) or (n_images, nz, ny, nx, 3) float32 as ModeImages.plane returns them; region (nz, ny, nx) or
None.  Chunk sums are vectorised over pairs, planes and chunks; the loop over a chunk's values is the stated sequential sum."""
import numpy as np

F4, F8 = np.float32, np.float64
NAN_BITS = 0x7FC00000
NAN = np.array([NAN_BITS], np.uint32).view(F4)[0]
CHUNK = 1024                                               # FROG_MODES_CHUNK
MAX_IMAGES = 512                                           # FROG_MODES_MAX_IMAGES


def support(planes, region=None):
    """bool (nz, ny, nx): region is non-zero and every image takes part (all components)."""
    p = np.ascontiguousarray(planes, F4)
    takes = p.view(np.uint32) != NAN_BITS
    if p.ndim == 5:
        takes = takes.all(axis=4)
    s = takes.all(axis=0)
    return s if region is None else s & (np.asarray(region) != 0)


def centre(planes, region=None):
    """(m, c, inside): m float64 value-shaped, c float64 (n,) + value shape with +0.0 outside the support, inside bool per
    value."""
    p = np.ascontiguousarray(planes, F4)
    n = len(p)
    inside = support(p, region)
    if p.ndim == 5:
        inside = np.repeat(inside[..., None], 3, axis=3)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(p.shape[1:], F8)
        for i in range(n):
            s = s + p[i].astype(F8)
        m = s / F8(n)
        c = np.where(inside[None], p.astype(F8) - m[None], F8(0.0))
    return m, c, inside


def gram(planes, region=None, gram=None, n_support=0):
    """(gram, n_support) as frog_modes_gram updates them: chunk sums, then the chunks of a plane, then the planes, ascending."""
    p = np.ascontiguousarray(planes, F4)
    n, nz = p.shape[0], p.shape[1]
    _, c, _ = centre(p, region)
    values = int(np.prod(p.shape[2:]))
    chunks = (values + CHUNK - 1) // CHUNK
    padded = np.zeros((n, nz, chunks * CHUNK), F8)
    padded[:, :, :values] = c.reshape(n, nz, values)
    padded = padded.reshape(n, nz, chunks, CHUNK)
    ii, jj = np.tril_indices(n)                              # row-major lower triangle: entry (i, j) at i (i + 1) / 2 + j
    sums = np.zeros((len(ii), nz, chunks), F8)
    for t in range(min(CHUNK, values)):
        prod = padded[ii, :, :, t] * padded[jj, :, :, t]
        sums = sums + prod
    g = np.zeros(len(ii), F8) if gram is None else np.array(gram, F8)
    for z in range(nz):
        t = np.zeros(len(ii), F8)
        for k in range(chunks):
            t = t + sums[:, z, k]
        g = g + t
    return g, int(n_support) + int(support(p, region).sum())


def project(planes, weights, region=None, fill=0.0):
    """(mean, modes) float32 as frog_modes_project stores them."""
    p = np.ascontiguousarray(planes, F4)
    w = np.ascontiguousarray(weights, F8).reshape(-1, len(p))
    m, c, inside = centre(p, region)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.where(inside, m.astype(F4), F4(fill))
        modes = np.empty((len(w),) + p.shape[1:], F4)
        for k in range(len(w)):
            s = np.zeros(p.shape[1:], F8)
            for i in range(len(p)):
                prod = w[k, i] * c[i]
                s = s + prod
            modes[k] = np.where(inside, s.astype(F4), F4(fill))
    return mean, modes


def unpack(g):
    """The symmetric matrix of a packed lower triangle."""
    g = np.asarray(g, F8)
    n = int(round((np.sqrt(8 * len(g) + 1) - 1) / 2))
    G = np.zeros((n, n), F8)
    G[np.tril_indices(n)] = g
    return G + np.tril(G, -1).T


def sign_rule(vectors):
    """Rows with their entry of largest magnitude (the lowest index on ties) made positive."""
    v = np.array(vectors, F8)
    for k in range(len(v)):
        if v[k, np.argmax(np.abs(v[k]))] < 0:
            v[k] = -v[k]
    return v


# ---- the designed case: 12 images on a 13 x 11 x 9 grid, 3 components ------------------------------------------------
DESIGNED_GRID = ((13, 11, 9), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))
DESIGNED_N, DESIGNED_SD = 12, (4.0, 2.0, 1.0)


def designed_case(seed=5):
    """(fields float32 (12, 9, 11, 13, 3), mean, psi (3, values) with rms 1 per value, B (12, 3)): field_i = mean + sum_k B_ik
    sd_k psi_k, psi orthogonal, B centred with orthogonal columns of norm sqrt(11): the sample covariance of the three
    coefficients is exactly the identity, so eigenvalue k is sd_k^2 x values, mode k is sd_k psi_k and the scores are B."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = DESIGNED_GRID[0]
    values = nx * ny * nz * 3
    psi = np.linalg.qr(rng.normal(size=(values, 3)))[0].T * np.sqrt(values)
    raw = rng.normal(size=(DESIGNED_N, 3))
    B = np.linalg.qr(raw - raw.mean(axis=0))[0] * np.sqrt(DESIGNED_N - 1.0)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mean = np.stack([2.0 * np.sin(x / 4.0), 1.5 * np.cos(y / 3.0), 0.1 * z], axis=3).reshape(-1)
    fields = mean[None] + (B * np.array(DESIGNED_SD)) @ psi
    return fields.astype(F4).reshape(DESIGNED_N, nz, ny, nx, 3), mean, psi, B


def plain_pca(fields):
    """Plain float64 PCA of the stored values: (eigenvalues (n,), modes (n, values) per s.d., scores (n, n) in s.d.), signs by
    the rule of frog_modes_eigen."""
    X = np.asarray(fields, F8).reshape(len(fields), -1)
    n = len(X)
    Xc = X - X.mean(axis=0)
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    flip = np.where(U[np.argmax(np.abs(U), axis=0), np.arange(n)] < 0, -1.0, 1.0)
    U, Vt = U * flip, Vt * flip[:, None]
    return s * s / (n - 1), Vt * (s / np.sqrt(n - 1.0))[:, None], U * np.sqrt(n - 1.0)
