"""fp64 numpy restatement of ``fd_backbone_oxygens`` and ``fd_dssp``, written from the rules and not
from the kernel, and by another route: a plain loop over the donors with the energies of all acceptors of one donor as
array expressions, the whole L x L energy matrix kept (``energies``), the kept bonds as a boolean matrix HB[acceptor, donor],
bridges and ladders as shifted copies of that matrix ANDed together, and the labels painted in the six passes the rules
name, in their order.  The kernel never holds a matrix: it keeps two acceptors per donor and gathers.

Indices are inside one chain of L residues; a chain is a float64 [L, 4, 3] array (N, CA, C, O per residue), an O row of
NaN marks a residue without oxygen.  Not collected by pytest (no ``test_`` prefix)."""
from itertools import groupby

import numpy as np

from psea_reference import rotation

O_ANGLE, O_LENGTH = 2.0992622, 1.2359372          # CA-C-O angle (rad) and C=O length (A) of the reference's script
Q = 27.888                                        # 0.084 e^2 * 332 kcal A / mol e^2
E_MIN, E_CUT, D_MIN, BEND = -9.9, -0.5, 0.5, 70.0
STATES = "-HBEGITS"
NO_DONOR, NO_ACCEPTOR = 1, 2
# the reference's NeRF constants: bond lengths N-CA, CA-C, C-N (A), bond angles N-CA-C, CA-C-N, C-N-CA (rad)
NERF_LENGTHS = (1.46, 1.54, 1.34)
NERF_ANGLES = (np.radians(109.0), np.radians(115.0), np.radians(121.0))


# ---------------------------------------------------------------------------------------------------- placement
def _cross(a, b):
    """Cross product along the last axis (np.cross spends most of its time on axis bookkeeping)."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def dihedral(a, b, c, d):
    """IUPAC dihedral of four points (rad); arrays of points give an array of dihedrals."""
    b0, b1, b2 = b - a, c - b, d - c
    n1, n2 = _cross(b0, b1), _cross(b1, b2)
    return np.arctan2((_cross(n1, n2) * _unit(b1)).sum(-1), (n1 * n2).sum(-1))


def place(a, b, c, angle, length, torsion):
    """The atom d bonded to c with |d - c| = length, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion; arrays of
    points (and of torsions) give an array of atoms."""
    bc = _unit(c - b)
    n = _unit(_cross(b - a, bc))
    m = _cross(n, bc)
    torsion = np.asarray(torsion)[..., None]
    return c + length * (-np.cos(angle) * bc + np.cos(torsion) * np.sin(angle) * m + np.sin(torsion) * np.sin(angle) * n)


def add_oxygens(nca_c, reference_torsion=False):
    """[L, 3, 3] (or [3L, 3]) N / CA / C -> [L, 4, 3] with O placed trans to the next N (``reference_torsion``: at the
    next N's own torsion, the reference script's literal call); NaN on the last residue.  All residues at once."""
    x = np.asarray(nca_c, np.float64).reshape(-1, 3, 3)
    out = np.full((len(x), 4, 3), np.nan)
    out[:, :3] = x
    if len(x) > 1:
        with np.errstate(invalid="ignore", divide="ignore"):
            psi = dihedral(x[:-1, 0], x[:-1, 1], x[:-1, 2], x[1:, 0])
            out[:-1, 3] = place(x[:-1, 0], x[:-1, 1], x[:-1, 2], O_ANGLE, O_LENGTH, psi if reference_torsion else psi + np.pi)
    return out


# ---------------------------------------------------------------------------------------------------- hydrogen bonds
def donors_acceptors(bb, flags=None):
    """(H positions [L, 3] with NaN for a non-donor, donor mask, acceptor mask)."""
    L = len(bb)
    flags = np.zeros(L, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    has_o = ~np.isnan(bb[:, 3]).any(1)
    H = np.full((L, 3), np.nan)
    donor = np.zeros(L, bool)
    for j in range(1, L):
        if flags[j] & NO_DONOR or not has_o[j - 1]:
            continue
        co = bb[j - 1, 2] - bb[j - 1, 3]
        n = np.sqrt((co * co).sum())
        if not n > 0.0:      # C and O on one point: no direction for the hydrogen
            continue
        H[j] = bb[j, 0] + co / n
        donor[j] = True
    acceptor = has_o & ((flags & NO_ACCEPTOR) == 0)
    return H, donor, acceptor


def donor_energies(bb, H, j, acceptor):
    """E of C=O(i) -> H-N(j) for every i at once, kcal/mol: float64 [L], NaN where the pair is not defined."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = [np.sqrt(((p - q) ** 2).sum(-1)) for p, q in
             ((bb[:, 3], bb[j, 0]), (bb[:, 2], H[j]), (bb[:, 3], H[j]), (bb[:, 2], bb[j, 0]))]   # ON, CH, OH, CN
        e = Q * (1.0 / d[0] + 1.0 / d[1] - 1.0 / d[2] - 1.0 / d[3])
        e = np.where(e < E_MIN, E_MIN, e)
        e = np.where((d[0] < D_MIN) | (d[1] < D_MIN) | (d[2] < D_MIN) | (d[3] < D_MIN), E_MIN, e)
    defined = acceptor.copy()
    defined[j] = False
    defined[j - 1] = False       # j >= 1 for every donor
    return np.where(defined, e, np.nan)


def energies(bb, flags=None):
    """float64 [L, L]: E[i, j] of acceptor i and donor j, NaN where the pair is not defined."""
    bb = np.asarray(bb, np.float64)
    L = len(bb)
    H, donor, acceptor = donors_acceptors(bb, flags)
    E = np.full((L, L), np.nan)
    for j in range(L):
        if donor[j]:
            E[:, j] = donor_energies(bb, H, j, acceptor)
    return E


def kept_bonds(E):
    """(acc int32 [L, 2], energy float64 [L, 2]): per donor the two acceptors of lowest E < -0.5, ties to the lower index."""
    L = E.shape[0]
    acc = np.full((L, 2), -1, np.int32)
    en = np.zeros((L, 2))
    for j in range(L):
        with np.errstate(invalid="ignore"):
            cand = sorted((E[i, j], i) for i in np.flatnonzero(E[:, j] < E_CUT))
        for k, (e, i) in enumerate(cand[:2]):
            acc[j, k], en[j, k] = i, e
    return acc, en


# ---------------------------------------------------------------------------------------------------- states
def bend_angles(bb):
    """Degrees [L], NaN where undefined: the angle between CA_i - CA_{i-2} and CA_{i+2} - CA_i."""
    ca = bb[:, 1]
    L = len(ca)
    out = np.full(L, np.nan)
    for i in range(2, L - 2):
        u, v = ca[i] - ca[i - 2], ca[i + 2] - ca[i]
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.dot(u, v) / (np.sqrt(np.dot(u, u)) * np.sqrt(np.dot(v, v)))
        out[i] = np.degrees(np.arccos(min(max(c, -1.0), 1.0))) if not np.isnan(c) else np.nan
    return out


def bridges(HB):
    """(parallel, antiparallel): boolean [L, L] matrices, symmetric, from HB[i, j] = hb(i, j); whole-matrix shifts."""
    L = len(HB)
    par, anti = np.zeros((L, L), bool), np.zeros((L, L), bool)
    if L < 5:
        return par, anti
    m = slice(1, L - 1)                   # i, j = 1 .. L-2
    lo, hi = slice(0, L - 2), slice(2, L)   # i-1 / j-1, i+1 / j+1
    T = HB.T
    # hb(i-1, j) & hb(j, i+1)  |  hb(j-1, i) & hb(i, j+1)
    par[m, m] = (HB[lo, m] & T[hi, m]) | (T[m, lo] & HB[m, hi])
    # hb(i, j) & hb(j, i)  |  hb(i-1, j+1) & hb(j-1, i+1)
    anti[m, m] = (HB[m, m] & T[m, m]) | (HB[lo, hi] & T[hi, lo])
    i, j = np.indices((L, L))
    far = np.abs(i - j) >= 3
    return par & far, anti & far


def _shift(M, di, dj):
    """S[i, j] = M[i + di, j + dj], False outside."""
    L = len(M)
    S = np.zeros_like(M)
    si, sj = slice(max(0, -di), L - max(0, di)), slice(max(0, -dj), L - max(0, dj))
    ti, tj = slice(max(0, di), L - max(0, -di)), slice(max(0, dj), L - max(0, -dj))
    S[si, sj] = M[ti, tj]
    return S


def assign(bb, acc):
    """The state codes int8 [L] from the kept bonds."""
    L = len(bb)
    HB = np.zeros((L, L), bool)
    for j in range(L):
        for a in acc[j]:
            if a >= 0:
                HB[a, j] = True
    lab = [0] * L

    def minimal(n):
        return [i for i in range(1, L - n) if HB[i - 1, i - 1 + n] and HB[i, i + n]]

    for i in minimal(4):                                                    # 1. H
        for k in range(i, i + 4):
            lab[k] = 1
    par, anti = bridges(HB)                                                 # 2. E, B
    ladder = (par & (_shift(par, 1, 1) | _shift(par, -1, -1))).any(1) | (anti & (_shift(anti, 1, -1) | _shift(anti, -1, 1))).any(1)
    bridge = par.any(1) | anti.any(1)
    for i in range(L):
        if not lab[i]:
            lab[i] = 3 if ladder[i] else 2 if bridge[i] else 0
    for n, code in ((3, 4), (5, 5)):                                        # 3. G, 4. I
        for i in minimal(n):
            if all(lab[k] in (0, code) for k in range(i, i + n)):
                for k in range(i, i + n):
                    lab[k] = code
    for n in (3, 4, 5):                                                     # 5. T
        for i in range(L - n):
            if HB[i, i + n]:
                for k in range(i + 1, i + n):
                    if lab[k] == 0:
                        lab[k] = 6
    bend = bend_angles(bb)                                                  # 6. S
    for i in range(2, L - 2):
        if lab[i] == 0 and bend[i] > BEND:
            lab[i] = 7
    return np.array(lab, np.int8)


def bridge_types(acc):
    """(has a parallel bridge, has an antiparallel bridge) of a chain's kept bonds."""
    L = len(acc)
    HB = np.zeros((L, L), bool)
    for j in range(L):
        for a in acc[j]:
            if a >= 0:
                HB[a, j] = True
    par, anti = bridges(HB)
    return bool(par.any()), bool(anti.any())


def dssp(bb, flags=None, E=None):
    """(state codes int8 [L], acc int32 [L, 2], energy float64 [L, 2], counts (kept bonds, runs of H, runs of E));
    ``E``: the chain's ``energies`` where they are already at hand."""
    bb = np.asarray(bb, np.float64)
    acc, en = kept_bonds(energies(bb, flags) if E is None else E)
    lab = assign(bb, acc)
    keys = [k for k, _ in groupby(lab.tolist())]
    return lab, acc, en, (int((acc >= 0).sum()), keys.count(1), keys.count(3))


def string(lab):
    return "".join(STATES[int(c)] for c in lab)


def threshold_margin(bb, flags=None, E=None):
    """The smallest of |E + 0.5| over all computed pairs, |bend - 70 degrees|, and the gap between the second- and
    third-best acceptor energies of any donor (inf where there is nothing to compare)."""
    bb = np.asarray(bb, np.float64)
    E = energies(bb, flags) if E is None else E
    m = np.inf
    v = E[~np.isnan(E)]
    if v.size:
        m = min(m, float(np.abs(v - E_CUT).min()))
    b = bend_angles(bb)
    b = b[~np.isnan(b)]
    if b.size:
        m = min(m, float(np.abs(b - BEND).min()))
    for j in range(len(bb)):
        with np.errstate(invalid="ignore"):
            col = np.sort(E[:, j][E[:, j] < E_CUT])
        if col.size >= 3:
            m = min(m, float(col[2] - col[1]))
    return m


# ---------------------------------------------------------------------------------------------------- test chains
def nerf_chain(phi, psi, omega=None):
    """[L, 3, 3] N / CA / C by NeRF placement with the reference's constants; phi[i], psi[i], omega[i] of residue i
    (phi[0] and the last psi / omega are not used)."""
    L = len(phi)
    omega = np.full(L, np.pi) if omega is None else omega
    (l_nca, l_cac, l_cn), (a_ncac, a_cacn, a_cnca) = NERF_LENGTHS, NERF_ANGLES
    x = np.zeros((L, 3, 3))
    x[0, 0] = (0.0, 0.0, 0.0)
    x[0, 1] = (l_nca, 0.0, 0.0)
    x[0, 2] = x[0, 1] + l_cac * np.array([-np.cos(a_ncac), np.sin(a_ncac), 0.0])
    for i in range(1, L):
        x[i, 0] = place(x[i - 1, 0], x[i - 1, 1], x[i - 1, 2], a_cacn, l_cn, psi[i - 1])
        x[i, 1] = place(x[i - 1, 1], x[i - 1, 2], x[i, 0], a_cnca, l_nca, omega[i - 1])
        x[i, 2] = place(x[i - 1, 2], x[i, 0], x[i, 1], a_ncac, l_cac, phi[i])
    return x


def ideal_chain(phi_deg, psi_deg, n=20):
    """n residues of one (phi, psi), with O: [n, 4, 3]."""
    return add_oxygens(nerf_chain(np.full(n, np.radians(phi_deg)), np.full(n, np.radians(psi_deg))))


SEGMENTS = {"alpha": (-57.0, -47.0), "g310": (-49.0, -26.0), "pi": (-57.0, -70.0), "beta": (-120.0, 130.0)}


# A second copy of an eight-residue extended strand (phi -120, psi 130, centred on its centroid) under x -> R x + t: the two
# placements a random search over rigid motions found to give the longest ladder of each bridge type with the first copy.
PAIR_PLACEMENT = {
    "parallel": ([[0.999437, 0.032754, -0.007329], [-0.032749, 0.999463, 0.000824], [0.007352, -0.000584, 0.999973]],
                 [2.762605, 2.897962, 0.431993]),
    "antiparallel": ([[-0.360686, -0.932244, 0.028749], [-0.774107, 0.316412, 0.548308], [-0.520254, 0.175512, -0.835782]],
                     [-1.83042, 3.770582, 0.868508]),
}


_STRAND = []


def strand_pair(kind):
    """[16, 3, 3]: two eight-residue extended strands side by side, the second straight after the first in the chain."""
    if not _STRAND:
        a = nerf_chain(np.full(8, np.radians(-120.0)), np.full(8, np.radians(130.0)))
        _STRAND.append(a - a.reshape(-1, 3).mean(0))
    a = _STRAND[0]
    R, t = PAIR_PLACEMENT[kind]
    return np.concatenate([a, a @ np.array(R).T + np.array(t)])


def segment_chain(rng, n, sigma):
    """n residues assembled from pieces of 3-24 residues, each under a random rotation and starting 3.8 A from the end
    of the one before: NeRF stretches of alpha, 3-10, pi, extended and random (phi, psi), and strand pairs of both
    bridge types; Gaussian noise of ``sigma`` A on N / CA / C, then O from ``add_oxygens``.  The idea of
    psea_reference.segment_chain for full backbones."""
    parts, total, end = [], 0, np.zeros(3)
    while total < n:
        kind = int(rng.integers(0, 8))
        k = int(rng.integers(3, 25))
        if kind < 4:
            p, q = SEGMENTS[("alpha", "g310", "pi", "beta")[kind]]
            x = nerf_chain(np.full(k, np.radians(p)), np.full(k, np.radians(q)))
        elif kind < 6:
            x = strand_pair(("parallel", "antiparallel")[kind - 4])
        else:
            x = nerf_chain(rng.uniform(-np.pi, np.pi, k), rng.uniform(-np.pi, np.pi, k))
        x = x[: n - total] @ rotation(rng).T
        step = rng.standard_normal(3)
        x = x - x[0, 0] + end + (3.8 * step / np.linalg.norm(step) if parts else 0.0)
        parts.append(x)
        end = x[-1, 2]
        total += len(x)
    x = np.concatenate(parts)
    return add_oxygens(x + rng.standard_normal(x.shape) * sigma)
