"""fp64 numpy restatement of the three further starts of ``fd_tm_align_ex`` (DESIGN.md "TM-align-style alignment"),
on top of ``tmalign_reference`` (starts 1 and 2, ``dp``, ``search``, ``threading``), with the decision margin extended
to the new decisions.  Not collected by pytest (no ``test_`` prefix).

Deliberately a different route, as there: SVD fits, whole score matrices through sqrt, plain loops over fragments.

The definition (shared with the header of csrc/tm_align_starts.hip and DESIGN.md).  x has n1 CA atoms, y has n2,
m = min(n1, n2), Ln >= m, d0 = d0(Ln), d01 = d0 + 1.5.  ``DP(S, g)``, ``search(map)`` and "refinement of a start map"
are those of ``tmalign_reference``.  The "fit of a set of pairs" is their least-squares superposition; the "fit score
of a map" is the TM sum of 1 / (1 + d^2 / d0^2) over the map's pairs under the fit of all its pairs, and -1 for a map
of fewer than 3 pairs.

* start 3, secondary structure plus distance: (R1, t1) = the fit of start 1's winning offset on its whole overlap (the
  fit that scored it; computed even when start 1 is not requested); S[i][j] = 1 / (1 + |R1 x_i + t1 - y_j|^2 / d01^2)
  + (0.5 if the P-SEA labels of x_i and y_j are equal, else 0); a0 = DP(S, -1).
* start 4, local superposition, only for m >= 12 (skipped below): fragment lengths f_a = min(20, m // 3) and
  f_b = min(100, m // 2), f_b only if f_b > f_a; for a length f and a chain of n residues the fragment positions are
  0, J, 2J, ... while position + f <= n, J = max(f, ceil((n - f + 1) / 8)) (at most 8 per chain, 64 pairs per length);
  the pairs are visited f_a before f_b, then the position in x ascending, then the position in y ascending; for each,
  (R, t) = the fit of x[i0 : i0 + f] onto y[j0 : j0 + f], S[i][j] = 1 / (1 + |R x_i + t - y_j|^2 / d01^2),
  map = DP(S, 0), value = the fit score of that map; a0 = the map with the largest value, the first on a tie.  At most
  128 programmes.
* start 5, fragment threading: a chain has a break after residue i if |c_{i+1} - c_i| >= 4.25 A; its longest stretch
  is the first longest run without a break; if neither chain has a break the start is skipped (it would equal start
  1); each chain that has a break and whose longest stretch has >= 4 residues has that stretch threaded, as a chain of
  its own, against the whole other chain by start 1's rule (the same overlap rule with the stretch's length in place
  of the chain's, scores under d0(Ln)), the indices shifted back; of the up to two maps the one with the higher
  threading score is a0, x's on a tie; no map, no start.
* result: every requested, non-skipped start is refined as starts 1 and 2 are; the candidate with the largest TM wins,
  the first on a tie, candidates in start order 1 .. 5, then g = -0.6 before 0, then iterations in order.  If every
  requested start is skipped there is no candidate: TM = -1, the identity transform and an empty map.

The decision margin (``margin`` of the result) is ``tmalign_reference``'s, extended: the best minus the best
fragment-pair value whose map differs (start 4, on the TM scale), the threading margins inside start 5 and its
x-against-y choice, every CA-CA step's distance from 4.25 A, and every cell of every traced DP path of starts 3
and 4."""
import functools

import numpy as np

import psea_reference as pr
import tm_reference as tr
import tmalign_reference as ta

START_NAMES = ("threading", "ss", "ss_dist", "local", "fragment")
BREAK = 4.25
MAX_FRAGMENT_POSITIONS = 8


def d01(Ln):
    return tr.d0(Ln) + 1.5


def labels(ca):
    return np.frombuffer(pr.psea(ca).encode(), np.uint8)


def distance_scores(x, y, R, t, scale):
    d = np.sqrt((((x @ R.T + t)[:, None, :] - y[None, :, :]) ** 2).sum(2))
    return 1.0 / (1.0 + (d / scale) ** 2)


def ss_dist_start(x, y, Ln):
    """(a0, margin): start 3."""
    a1, _ = ta.threading(x, y, Ln)
    i = np.flatnonzero(a1 >= 0)
    R1, t1 = tr.kabsch(x[i], y[a1[i]])
    S = distance_scores(x, y, R1, t1, d01(Ln)) + 0.5 * (labels(x)[:, None] == labels(y)[None, :])
    return ta.dp(S, -1.0)


def fragment_positions(n, f):
    J = max(f, -(-(n - f + 1) // MAX_FRAGMENT_POSITIONS))
    return list(range(0, n - f + 1, J))


def fragment_lengths(m):
    fa, fb = min(20, m // 3), min(100, m // 2)
    return [fa, fb] if fb > fa else [fa]


def fit_score(x, y, amap, Ln):
    """The TM sum of the map's pairs under the fit of all its pairs, on the TM scale (divided by Ln); -1 below 3
    pairs."""
    xa, ya = ta.aligned(x, y, amap)
    if len(xa) < 3:
        return -1.0
    R, t = tr.kabsch(xa, ya)
    return tr.tm_of(xa, ya, R, t, Ln=Ln)


def local_start(x, y, Ln):
    """(a0 or None when skipped, margin, number of programmes): start 4."""
    n1, n2 = len(x), len(y)
    m = min(n1, n2)
    if m < 12:
        return None, np.inf, 0
    margin = np.inf
    cands = []
    for f in fragment_lengths(m):
        for i0 in fragment_positions(n1, f):
            for j0 in fragment_positions(n2, f):
                R, t = tr.kabsch(x[i0:i0 + f], y[j0:j0 + f])
                amap, mg = ta.dp(distance_scores(x, y, R, t, d01(Ln)), 0.0)
                margin = min(margin, mg)
                cands.append((fit_score(x, y, amap, Ln), amap))
    assert len(cands) <= 128
    b = int(np.argmax([v for v, _ in cands]))   # the first of the largest
    for v, amap in cands:
        if not np.array_equal(amap, cands[b][1]):
            margin = min(margin, cands[b][0] - v)
    return cands[b][1], float(margin), len(cands)


def steps(ca):
    return np.sqrt((np.diff(ca, axis=0) ** 2).sum(1))


def longest_stretch(ca):
    """(start, length of the first longest run without a break, whether the chain has a break)."""
    brk = steps(ca) >= BREAK
    best, start = (0, 0), 0
    for i in range(len(ca)):
        if i == len(ca) - 1 or brk[i]:
            if i + 1 - start > best[1]:
                best = (start, i + 1 - start)
            start = i + 1
    return best[0], best[1], bool(brk.any())


def break_margin(ca):
    s = steps(ca)
    return float(np.abs(s - BREAK).min()) if s.size else np.inf


def fragment_start(x, y, Ln):
    """(a0 or None when skipped, margin): start 5."""
    n1 = len(x)
    sx, lx, bx = longest_stretch(x)
    sy, ly, by = longest_stretch(y)
    margin = min(break_margin(x), break_margin(y))
    maps = []   # (score, map), x's first
    if bx and lx >= 4:
        sub, mg = ta.threading(x[sx:sx + lx], y, Ln)
        margin = min(margin, mg)
        amap = np.full(n1, -1, np.int64)
        amap[sx:sx + lx] = sub
        maps.append((threading_score(x, y, amap, Ln), amap))
    if by and ly >= 4:
        sub, mg = ta.threading(x, y[sy:sy + ly], Ln)
        margin = min(margin, mg)
        amap = np.where(sub >= 0, sub + sy, -1)
        maps.append((threading_score(x, y, amap, Ln), amap))
    if not maps:
        return None, margin
    if len(maps) == 2 and not np.array_equal(maps[0][1], maps[1][1]):
        margin = min(margin, abs(maps[0][0] - maps[1][0]))
    return (maps[0][1] if len(maps) == 1 or maps[0][0] >= maps[1][0] else maps[1][1]), float(margin)


def threading_score(x, y, amap, Ln):
    """The score start 1's rule gave the gapless map: the TM sum under the fit on its whole overlap."""
    xa, ya = ta.aligned(x, y, amap)
    R, t = tr.kabsch(xa, ya)
    return tr.tm_of(xa, ya, R, t, Ln=Ln)


def selection(starts):
    """The tuple of start names in start order for ``starts`` (names, "all", or a bit set)."""
    if isinstance(starts, (int, np.integer)):
        return tuple(n for b, n in enumerate(START_NAMES) if starts >> b & 1)
    if starts == "all":
        return START_NAMES
    return tuple(n for n in START_NAMES if n in starts)


def tm_align(x, y, Ln=None, max_iter=10, starts="all"):
    """``tmalign_reference.tm_align`` with the five starts: the same dict, ``start_tms`` a float [5] array with -1
    where a start was not requested or was skipped, and ``programmes`` the number of DPs of start 4."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n1, n2 = len(x), len(y)
    Ln = n2 if Ln is None else int(Ln)
    assert n1 >= 1 and n2 >= 1 and Ln >= min(n1, n2) and max_iter >= 1
    sel = selection(starts)
    assert sel
    margin = np.inf
    best = None
    n_cand = 0
    programmes = 0
    start_tms = np.full(5, -1.0)

    def offer(tm, R, t, amap):
        nonlocal best, margin, n_cand
        n_cand += 1
        if best is None:
            best = (tm, R, t, amap)
            return
        if not np.array_equal(amap, best[3]):
            margin = min(margin, abs(tm - best[0]))
        if tm > best[0]:
            best = (tm, R, t, amap)

    for s, name in enumerate(START_NAMES):
        if name not in sel:
            continue
        if name == "threading":
            a0, mg = ta.threading(x, y, Ln)
        elif name == "ss":
            a0, mg = ta.ss_start(x, y), np.inf
        elif name == "ss_dist":
            a0, mg = ss_dist_start(x, y, Ln)
            mg = min(mg, ta.threading(x, y, Ln)[1])
        elif name == "local":
            a0, mg, programmes = local_start(x, y, Ln)
        else:
            a0, mg = fragment_start(x, y, Ln)
        margin = min(margin, mg)
        if a0 is None:
            continue
        tm0, R0, t0 = ta.search(x, y, a0, Ln)
        offer(tm0, R0, t0, a0)
        reached = tm0
        for g in ta.GAP_OPENS:
            R, t, prev = R0, t0, a0
            for _ in range(max_iter):
                amap, mg = ta.dp(ta.score_matrix(x, y, R, t, Ln), g)
                margin = min(margin, mg)
                if np.array_equal(amap, prev):
                    break
                tm, R, t = ta.search(x, y, amap, Ln)
                offer(tm, R, t, amap)
                reached = max(reached, tm)
                prev = amap
        start_tms[s] = reached
    if best is None:   # no requested start applies to the pair
        best = (-1.0, np.eye(3), np.zeros(3), np.full(n1, -1, np.int64))
    tm, R, t, amap = best
    return dict(tm=tm, R=R, t=t, map=amap, n_ali=int((amap >= 0).sum()), margin=float(margin), candidates=n_cand,
                start_tms=start_tms, programmes=programmes)


# ---------------------------------------------------------------------------------------------------- test pairs
def rehinged_pair(rng, n):
    """Two domains, the second re-hinged (a random rotation about the hinge residue, moved 6-12 A) and an insertion of
    4-9 residues in the first: no single gapless offset or label programme covers both, a fragment fit finds one."""
    a = tr.ca_chain(rng, n)
    h = n // 2 + int(rng.integers(-3, 4))
    b = tr.two_domain(a, h, angle_deg=float(rng.uniform(60, 150)), shift=float(rng.uniform(6, 12)), axis=rng.standard_normal(3))
    k = int(rng.integers(4, 10))
    s = int(rng.integers(3, h - 3))
    loop = b[s - 1] + tr.ca_chain(rng, k + 1)[1:]
    b = np.concatenate([b[:s], loop, b[s:] + (loop[-1] - b[s - 1])])
    return a, ta._move(rng, b + rng.standard_normal(b.shape) * 0.3)


def broken(rng, a, n_breaks):
    """``a`` with ``n_breaks`` chain breaks: from each break on, the rest is moved so that the step there is 6-10 A."""
    a = a.copy()
    at = sorted(rng.choice(np.arange(4, len(a) - 4), n_breaks, replace=False))
    for i in at:
        d = a[i + 1] - a[i]
        a[i + 1:] += d / np.linalg.norm(d) * (float(rng.uniform(6, 10)) - np.linalg.norm(d))
    return a


def break_pair(rng, n, where):
    """A chain and a shorter, slightly noisy copy of it, with one or two breaks in x, in y or in both."""
    a = tr.ca_chain(rng, n)
    cut = int(rng.integers(2, max(3, n // 6)))
    b = a[cut:] + rng.standard_normal((n - cut, 3)) * 0.2
    if where in ("x", "both"):
        a = broken(rng, a, int(rng.integers(1, 3)))
    if where in ("y", "both"):
        b = broken(rng, b, int(rng.integers(1, 3)))
    return a, ta._move(rng, b)


def unbroken_pair(rng, n):
    """A chain and a truncated copy with 0.05 A noise: every step stays at 3.8 A, so start 5 is skipped."""
    a = tr.ca_chain(rng, n)
    b = a[3:n - 2] + rng.standard_normal((n - 5, 3)) * 0.05
    return a, ta._move(rng, b)


def _attach(rng, prev, seg):
    """``seg`` moved so that it starts 3.8 A from the end of ``prev``, appended."""
    u = rng.standard_normal(3)
    return np.concatenate([prev, seg - seg[0] + prev[-1] + 3.8 * u / np.linalg.norm(u)])


def core_pair(rng, c, p1, q1, p2, q2):
    """Two chains that share a core of ``c`` residues (0.3 A noise, rotated) between unrelated flanks of p1, q1 and p2,
    q2 residues: the gapless fit on a whole overlap is diluted by the flanks, a fragment inside the core is not."""
    core = tr.ca_chain(rng, c)
    a = _attach(rng, _attach(rng, tr.ca_chain(rng, p1), core), tr.ca_chain(rng, q1))
    moved = core @ tr.rotation(rng).T + rng.standard_normal(core.shape) * 0.3
    b = _attach(rng, _attach(rng, tr.ca_chain(rng, p2), moved), tr.ca_chain(rng, q2))
    return a, ta._move(rng, b)


SEED = 20250301


@functools.lru_cache(maxsize=None)
def parity_set():
    """The seeded pairs of the all-starts parity tests: [(kind, a, b, Ln or None, max_iter)], 28 pairs of lengths 8-136
    and one 300 x 200 pair at max_iter = 2."""
    rng = np.random.default_rng(SEED)
    out = []
    for n in (30, 97):
        a, b, _ = ta.deletion_pair(rng, n)
        out.append(("deletion", a, b + rng.standard_normal(b.shape) * 0.3, None, 10))
        a, b = ta.insertion_pair(rng, n + 5)
        out.append(("insertion", a, b, len(b) + 7 if n == 30 else None, 10))
        a, b = ta.hinge_pair(rng, n + 11, noise=0.5)
        out.append(("hinge", a, b, None, 10))
    for n1, n2 in ((40, 75), (130, 52), (88, 91), (64, 110)):
        out.append(("unrelated",) + ta.unrelated_pair(rng, n1, n2) + (None, 10))
    for n in (48, 64, 80, 96, 113):
        out.append(("rehinged",) + rehinged_pair(rng, n) + (None, 10))
    for c, p1, q1, p2, q2 in ((30, 40, 12, 8, 50), (36, 10, 60, 45, 20), (42, 55, 30, 12, 70)):
        out.append(("core",) + core_pair(rng, c, p1, q1, p2, q2) + (None, 10))
    for q, n in enumerate((36, 55, 70, 84, 101, 120)):
        out.append(("break_" + ("x", "y", "both")[q % 3],) + break_pair(rng, n, ("x", "y", "both")[q % 3]) + (None, 10))
    a, b = unbroken_pair(rng, 16)
    out.append(("short", a[:9], b, None, 10))            # m = 9: start 4 skipped
    a, b = ta.insertion_pair(rng, 8)
    out.append(("short", a, b, None, 10))                # m = 8
    for n in (33, 77):
        out.append(("unbroken",) + unbroken_pair(rng, n) + (None, 10))
    out.append(("unrelated",) + ta.unrelated_pair(rng, 300, 200) + (None, 2))
    return out


@functools.lru_cache(maxsize=None)
def parity_results():
    """``tm_align(starts="all")`` of every pair of ``parity_set()``, once per process (read-only)."""
    return [tm_align(a, b, Ln=Ln, max_iter=it) for _, a, b, Ln, it in parity_set()]


@functools.lru_cache(maxsize=None)
def parity_results_two():
    """The same pairs with starts 1 and 2 only."""
    return [tm_align(a, b, Ln=Ln, max_iter=it, starts=("threading", "ss")) for _, a, b, Ln, it in parity_set()]
