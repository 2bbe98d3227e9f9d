"""fp64 numpy restatement of the TM-score search of ``fd_tm_score`` (DESIGN.md "TM-score"), vectorised over seeds.

Deliberately a different route to the same definition: fits by SVD with a determinant correction (the kernel uses
Horn's quaternion eigenvector), two-pass centred covariances, distances through sqrt, the selection compared as a set,
and the widened cutoff found by counting up j = 1, 2, ...  Not collected by pytest (no ``test_`` prefix)."""
import numpy as np

MAX_SEL_FITS = 20


def d0(Ln):
    return 1.24 * np.cbrt(Ln - 15) - 1.8 if Ln > 21 else 0.5


def seeds(n, stride=1):
    """(length, start) of every seed in search order: lengths descending, starts ascending."""
    lmin = min(n, 4)
    lengths = []
    l = n
    while l > lmin:
        lengths.append(l)
        l //= 2
    lengths.append(lmin)
    out = []
    for l in lengths:
        starts = list(range(0, n - l + 1, stride))
        if starts[-1] != n - l:
            starts.append(n - l)
        out += [(l, s) for s in starts]
    return out


def fit(x, y, w):
    """Least-squares rigid fits y ~ R x + t over the residues selected by each row of the boolean ``w`` [S, n]:
    R [S, 3, 3] (proper rotations), t [S, 3]."""
    wf = w.astype(np.float64)
    m = wf.sum(1)
    cx = wf @ x / m[:, None]
    cy = wf @ y / m[:, None]
    u = x[None] - cx[:, None]
    v = y[None] - cy[:, None]
    H = np.einsum("sn,sni,snj->sij", wf, u, v)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("sji,skj->sik", Vt, U)))
    d[d == 0] = 1.0
    D = np.zeros((len(w), 3, 3))
    D[:, 0, 0] = 1.0
    D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = np.einsum("sji,sjk,slk->sil", Vt, D, U)   # V D U^T
    t = cy - np.einsum("sij,sj->si", R, cx)
    return R, t


def tm_search(x, y, Ln=None, stride=1):
    """(TM-score, R, t) of the residue-paired traces x, y [n, 3]: the largest TM(T_k) over all seeds and iterations,
    the first in seed order, then iteration order, on a tie."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n = len(x)
    Ln = n if Ln is None else Ln
    assert Ln >= n >= 1
    dd0 = d0(Ln)
    dcut = min(max(dd0, 4.5), 8.0)
    need = min(3, n)
    sd = seeds(n, stride)
    S = len(sd)
    idx = np.arange(n)
    sel = np.array([(idx >= s) & (idx < s + l) for l, s in sd])
    R, t = fit(x, y, sel)
    best = np.full(S, -np.inf)
    bR, bt = R.copy(), t.copy()
    active = np.ones(S, bool)
    for k in range(MAX_SEL_FITS + 1):
        d = np.sqrt((((x[None] @ np.transpose(R, (0, 2, 1))) + t[:, None] - y[None]) ** 2).sum(2))
        tm = (1.0 / (1.0 + (d / dd0) ** 2)).sum(1) / Ln
        up = active & (tm > best)
        best[up], bR[up], bt[up] = tm[up], R[up], t[up]
        if k == MAX_SEL_FITS:
            break
        c = np.full(S, dcut)
        new = d < c[:, None]
        short = new.sum(1) < need
        j = 0
        while short.any():
            j += 1
            c[short] = dcut + 0.5 * j
            new[short] = d[short] < c[short, None]
            short = new.sum(1) < need
        active &= ~(new == sel).all(1)
        if not active.any():
            break
        sel = np.where(active[:, None], new, sel)
        R2, t2 = fit(x, y, sel[active])
        R[active], t[active] = R2, t2
    i = int(np.argmax(best))
    return float(best[i]), bR[i], bt[i]


def tm_of(x, y, R, t, Ln=None):
    """TM(R, t) of the pair, normalised by Ln (default n)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    Ln = len(x) if Ln is None else Ln
    d = np.sqrt(((x @ np.asarray(R).T + t - y) ** 2).sum(1))
    return float((1.0 / (1.0 + (d / d0(Ln)) ** 2)).sum() / Ln)


def kabsch(x, y):
    """The all-residue least-squares fit (R, t)."""
    R, t = fit(np.asarray(x, np.float64), np.asarray(y, np.float64), np.ones((1, len(x)), bool))
    return R[0], t[0]


def rotation(rng):
    q = rng.standard_normal(4)
    w, a, b, c = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                     [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                     [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])


def ca_chain(rng, n, step=3.8):
    """A CA-like trace: a self-avoiding-ish random walk of 3.8 A steps with a persistent direction."""
    out = np.zeros((n, 3))
    d = rng.standard_normal(3)
    d /= np.linalg.norm(d)
    for i in range(1, n):
        d = d + rng.standard_normal(3) * 0.6
        d /= np.linalg.norm(d)
        out[i] = out[i - 1] + step * d
    return out


def two_domain(a, hinge, angle_deg=90.0, shift=10.0, axis=(0.0, 0.0, 1.0)):
    """b: residues < hinge equal a; the rest rotated by angle_deg about ``axis`` through residue ``hinge`` and moved
    ``shift`` A along the axis."""
    th = np.deg2rad(angle_deg)
    k = np.asarray(axis, np.float64)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rh = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    b = a.copy()
    p = a[hinge]
    b[hinge:] = (a[hinge:] - p) @ Rh.T + p + shift * k
    return b
