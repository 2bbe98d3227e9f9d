"""fp64 numpy restatement of the P-SEA annotation of ``fd_annotate_sse`` (DESIGN.md "Secondary structure (P-SEA)"),
with its internals exposed: the per-residue quantities, the flags, the runs, the contact sums, and the distance of a
chain from every threshold.

Deliberately a different route to the same definition: whole-chain array slices, the dihedral through the cross
product of the two plane normals, all n x n distances through sqrt, runs found by a scan over the mask, and the labels
scattered in the two passes the definition names (the kernel gathers them).  Angles are in degrees, distances in A.
Not collected by pytest (no ``test_`` prefix)."""
from itertools import groupby

import numpy as np

HELIX = {"d3": [(4.8, 5.8)], "d4": [(5.8, 7.0)], "r": [(77.0, 101.0)], "a": [(30.0, 70.0)]}
STRAND = {"d2": [(6.1, 7.3)], "d3": [(9.0, 10.8)], "d4": [(11.3, 13.5)], "r": [(110.0, 138.0)],
          "a": [(-180.0, -125.0), (145.0, 180.0)]}
CONTACT = (4.2, 5.2)


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def geometry(ca):
    """d2, d3, d4 (A), r, a (degrees) per residue as float64 [n] arrays; NaN where a quantity is undefined."""
    x = np.asarray(ca, np.float64).reshape(-1, 3)
    n = len(x)
    q = {k: np.full(n, np.nan) for k in ("d2", "d3", "d4", "r", "a")}
    if n >= 3:
        q["d2"][1:n - 1] = _norm(x[2:] - x[:-2])
        u, v = x[:-2] - x[1:-1], x[2:] - x[1:-1]
        q["r"][1:n - 1] = np.degrees(np.arccos(np.clip((u * v).sum(-1) / (_norm(u) * _norm(v)), -1.0, 1.0)))
    if n >= 4:
        q["d3"][1:n - 2] = _norm(x[3:] - x[:-3])
        b0, b1, b2 = x[1:-2] - x[:-3], x[2:-1] - x[1:-2], x[3:] - x[2:-1]
        n1, n2 = np.cross(b0, b1), np.cross(b1, b2)
        y = (np.cross(n1, n2) * (b1 / _norm(b1)[:, None])).sum(-1)
        q["a"][1:n - 2] = np.degrees(np.arctan2(y, (n1 * n2).sum(-1)))
    if n >= 5:
        q["d4"][1:n - 3] = _norm(x[4:] - x[:-4])
    return q


def _in(table, q, name):
    """Closed-range test of q[name] against the class's ranges; false where the quantity is undefined (NaN)."""
    v = q[name]
    with np.errstate(invalid="ignore"):
        out = np.zeros(len(v), bool)
        for lo, hi in table[name]:
            out |= (v >= lo) & (v <= hi)
    return out


def flags(ca):
    """Boolean [n] arrays: potential helix, potential strand, helix extension test, strand extension test."""
    q = geometry(ca)
    h3, hr = _in(HELIX, q, "d3"), _in(HELIX, q, "r")
    s3 = _in(STRAND, q, "d3")
    ph = (h3 & _in(HELIX, q, "d4")) | (hr & _in(HELIX, q, "a"))
    ps = (_in(STRAND, q, "d2") & s3 & _in(STRAND, q, "d4")) | (_in(STRAND, q, "r") & _in(STRAND, q, "a"))
    return ph, ps, h3 | hr, s3


def distances(ca):
    x = np.asarray(ca, np.float64).reshape(-1, 3)
    return _norm(x[:, None] - x[None])


def contacts(ca):
    """Per residue, the number of residues of the chain at 4.2 ... 5.2 A."""
    D = distances(ca)
    return ((D >= CONTACT[0]) & (D <= CONTACT[1])).sum(1)


def runs(mask):
    """(start, end) of every maximal run of True in ``mask``, end exclusive."""
    out, start = [], None
    for i, m in enumerate(list(mask) + [False]):
        if m and start is None:
            start = i
        elif not m and start is not None:
            out.append((start, i))
            start = None
    return out


def three_run_sums(ca):
    """The contact sum of every potential-strand run of length exactly 3, in chain order."""
    c = contacts(ca)
    return [int(c[s:e].sum()) for s, e in runs(flags(ca)[1]) if e - s == 3]


def sets(ca):
    """Boolean [n] arrays: the helix residues and the strand residues of steps 1 and 2."""
    ph, ps, _, _ = flags(ca)
    n = len(ph)
    helix, strand = np.zeros(n, bool), np.zeros(n, bool)
    for s, e in runs(ph):
        if e - s >= 5:
            helix[s:e] = True
    c = contacts(ca)
    for s, e in runs(ps):
        if e - s >= 4 or (e - s == 3 and c[s:e].sum() >= 5):
            strand[s:e] = True
    return helix, strand


def label_passes(ca):
    """(labels after the helix pass, labels after the strand pass), each a list of 'a' / 'b' / 'c'."""
    _, _, eh, es = flags(ca)
    helix, strand = sets(ca)
    n = len(eh)
    sse = ["c"] * n
    for i in np.flatnonzero(helix):
        sse[i] = "a"
        if i > 0 and eh[i - 1]:
            sse[i - 1] = "a"
        if i + 1 < n and eh[i + 1]:
            sse[i + 1] = "a"
    first = list(sse)
    for i in np.flatnonzero(strand):
        sse[i] = "b"
        if i > 0 and es[i - 1]:
            sse[i - 1] = "b"
        if i + 1 < n and es[i + 1]:
            sse[i + 1] = "b"
    return first, sse


def psea(ca) -> str:
    """The label string of one CA trace [n, 3]."""
    return "".join(label_passes(ca)[1])


def counts(sse):
    """(n_alpha, n_beta): the number of maximal runs of 'a' and of 'b'."""
    keys = [k for k, _ in groupby(sse)]
    return keys.count("a"), keys.count("b")


def threshold_margin(ca) -> float:
    """The smallest distance of any defined d2 / d3 / d4 / r / a, and of any CA-CA distance of the chain, from any
    threshold it is tested against (A or degrees); inf for a chain with nothing to test."""
    q = geometry(ca)
    m = np.inf
    for table in (HELIX, STRAND):
        for name, ranges in table.items():
            v = q[name][~np.isnan(q[name])]
            if v.size:
                m = min(m, min(np.abs(v - t).min() for r in ranges for t in r))
    D = distances(ca)
    if D.size:
        m = min(m, min(np.abs(D - t).min() for t in CONTACT))
    return float(m)


# ---------------------------------------------------------------------------------------------------- test chains
def rotation(rng):
    q = rng.standard_normal(4)
    w, a, b, c = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                     [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                     [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])


def ideal_helix(n):
    i = np.arange(n)
    return np.stack([2.3 * np.cos(np.radians(100.0) * i), 2.3 * np.sin(np.radians(100.0) * i), 1.5 * i], 1)


def flat_strand(n, y=0.0):
    """Rise 3.3 A, zig-zag +-0.9 A, exactly planar (every dihedral is +-180 degrees)."""
    j = np.arange(n)
    return np.stack([3.3 * j, np.full(n, y), 0.9 * (-1.0) ** j], 1)


def wavy_strand(n):
    """The same strand with a 0.3 A wave across it, so that no dihedral is exactly +-180 degrees."""
    j = np.arange(n)
    return np.stack([3.3 * j, 0.3 * np.sin(1.3 * j), 0.9 * (-1.0) ** j], 1)


def hairpin():
    """Two antiparallel 10-residue flat strands 4.8 A apart, joined by two turn residues."""
    turn = np.array([[31.5, 1.6, 2.5], [32.0, 3.3, 5.0]])
    return np.concatenate([flat_strand(10, 0.0), turn, flat_strand(10, 4.8)[::-1]])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def random_walk(rng, n):
    p = np.zeros((n, 3))
    for k in range(1, n):
        p[k] = p[k - 1] + 3.8 * _unit(rng)
    return p


def segment_chain(rng, n, sigma):
    """n residues assembled from ideal-helix, wavy-strand and 3.8 A random-walk segments of 3-24 residues, each under
    a random rotation and starting 3.8 A from the end of the one before, plus Gaussian noise of ``sigma`` A."""
    parts, total, end = [], 0, np.zeros(3)
    while total < n:
        k = min(int(rng.integers(3, 25)), n - total)
        kind = int(rng.integers(0, 3))
        s = (ideal_helix(k) if kind == 0 else wavy_strand(k) if kind == 1 else random_walk(rng, k)) @ rotation(rng).T
        s = s - s[0] + end + (3.8 * _unit(rng) if parts else 0.0)
        parts.append(s)
        end = s[-1]
        total += k
    ca = np.concatenate(parts)
    return ca + rng.standard_normal(ca.shape) * sigma
