"""The clash count and the lDDT as numpy statements of the rules in DESIGN.md "Clash counts and lDDT" -- the yardstick
of tests/test_clash_lddt.py and tests/test_clash_lddt_gpu.py, in the role tests/psea_reference.py has for P-SEA.

Coordinates are taken as float32 (what a PDB file holds) and widened to float64 before the first subtraction; a
distance is sqrt(dx dx + dy dy + dz dz).  Each function also returns its *margin*: the smallest distance of any decision
it made from that decision's threshold.  The tests only use inputs whose margin is >= MIN_MARGIN: a float64 distance is
rounded by about 1e-15, so with that margin the integers cannot depend on how a square root or a fused multiply-add
rounds, and the device's integers can be compared with ``==``."""
import numpy as np

MIN_MARGIN = 1e-9
RADII = np.array([1.55, 1.7, 1.7])   # N, CA, C
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def _distances(x):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def clashes(xyz, alpha=0.63):
    """(count, bool flags [3n], margin) of a backbone [3n, 3] (N, CA, C per residue): atoms a, b clash iff |a - b| >= 2
    and d(a, b) <= alpha (r_a + r_b); the count is the number of atoms that clash with at least one other."""
    d = _distances(xyz)
    n = len(d)
    r = RADII[np.arange(n) % 3]
    limit = alpha * (r[:, None] + r[None, :])
    idx = np.arange(n)
    apart = np.abs(idx[:, None] - idx[None, :]) >= 2
    hit = apart & (d <= limit)
    flags = hit.any(axis=1)
    margin = np.abs(d - limit)[apart].min() if apart.any() else np.inf
    return int(flags.sum()), flags, float(margin)


def lddt_counts(model, ref, atoms_per_res=3, radius=15.0, thresholds=THRESHOLDS):
    """((conserved, total), int64 [n_res, 2] of the same per residue, margin) of a model against a reference, both
    [A n, 3].  An unordered pair of atoms of different residues is included iff d_ref < radius; an included pair is
    conserved at tau iff |d_model - d_ref| < tau; conserved is summed over the thresholds."""
    A = atoms_per_res
    dm, dr = _distances(model), _distances(ref)
    n = len(dr)
    assert dm.shape == dr.shape and n % A == 0
    res = np.arange(n) // A
    other = res[:, None] != res[None, :]
    included = other & (dr < radius)
    delta = np.abs(dm - dr)
    kept = np.zeros((n, n), dtype=np.int64)
    margin = np.abs(dr - radius)[other].min() if other.any() else np.inf
    for tau in thresholds:
        kept += included & (delta < tau)
        if included.any():
            margin = min(margin, np.abs(delta - tau)[included].min())
    atom = np.stack([kept.sum(axis=1), included.sum(axis=1)], axis=1)       # ordered pairs of each atom
    per_res = atom.reshape(n // A, A, 2).sum(axis=1)
    total = atom.sum(axis=0)
    assert (total % 2 == 0).all()
    return (int(total[0] // 2), int(total[1] // 2)), per_res, float(margin)


def score(conserved, total, n_thresholds=len(THRESHOLDS)):
    return conserved / (n_thresholds * total) if total > 0 else float("nan")


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def walk_backbone(rng, n_res, jitter=0.45):
    """float32 [3 n_res, 3]: a chain of atoms about 1.45 A apart whose direction drifts slowly (so atoms two apart sit
    near 2.6 A, above every clash limit), then moved by N(0, jitter) per coordinate so that some atoms clash and some
    do not."""
    n = 3 * n_res
    step = rng.standard_normal(3)
    steps = np.empty((n, 3))
    for i in range(n):
        step = step / np.linalg.norm(step) + 0.55 * rng.standard_normal(3)
        steps[i] = 1.45 * step / np.linalg.norm(step)
    x = np.cumsum(steps, axis=0) + jitter * rng.standard_normal((n, 3))
    return x.astype(np.float32)


def jittered_model(rng, ref):
    """float32 model of ``ref``: every atom moved by N(0, s) per coordinate with its own s between 0.3 and 3 A, so that
    each of the four default thresholds is passed by some pairs and missed by others."""
    ref = np.asarray(ref, dtype=np.float32)
    s = rng.uniform(0.3, 3.0, size=(len(ref), 1))
    return (ref.astype(np.float64) + s * rng.standard_normal(ref.shape)).astype(np.float32)
