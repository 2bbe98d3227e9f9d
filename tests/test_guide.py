"""Restraint guidance without a device: the derivative's formula (tests/guide_reference.py) against torch autograd, the
restraint builders and their packed layout, the guidance coefficients, the rejections of the model-free entries (checked on
the host before any device call), and a descent that uses the reference statement alone."""
import ctypes as C

import numpy as np
import pytest

import guide_reference as gr
from foldingdiff_amd import beta_schedules, sampling, structures

NAMES9 = ["phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA", "0C:1N", "N:CA", "CA:C"]
IDX = {3: np.array([0, 1, 2, -1, -1, -1, -1, -1, -1], np.int32), 6: np.array([0, 1, 2, 3, 4, 5, -1, -1, -1], np.int32),
       9: np.arange(9, dtype=np.int32)}
MOTIF_RES = [2, 5, 8, 11, 15, 18, 21, 23]


def random_features(rng, n, F) -> np.ndarray:
    """float32 [n, F] in the column order of NAMES9: torsions anywhere on the circle, bond angles and lengths near a backbone's."""
    cols = [rng.uniform(-np.pi, np.pi, n) for _ in range(3)]
    cols += [m + 0.1 * rng.standard_normal(n) for m in (1.94, 2.03, 2.12)]
    cols += [m + 0.03 * rng.standard_normal(n) for m in (1.33, 1.46, 1.52)]
    return np.stack(cols[:F], axis=1).astype(np.float32)


SIN_FLOOR = 0.02
DOMAIN_MODES = ("signs", "negative", "backbone")


def domain_features(rng, n, F, mode="signs") -> np.ndarray:
    """float32 [n, F] over the whole domain of the NeRF forward, in the column order of NAMES9.  Torsions uniform on the circle.
    ``mode`` "signs": each bond angle uniform in [asin(SIN_FLOOR), pi - asin(SIN_FLOOR)] (both sides of pi / 2) times a random
    sign, each length as random_features' times a random sign; "negative": the same magnitudes, every bond angle negative,
    lengths positive; "backbone": random_features.  sin(angle) == 0 and length == 0 stay out: behind such an atom the forward
    itself is not finite (the next frame's cross product vanishes)."""
    if mode == "backbone":
        return random_features(rng, n, F)
    assert mode in DOMAIN_MODES, mode
    lo = np.arcsin(SIN_FLOOR)
    sign = (lambda: rng.choice([-1.0, 1.0], n)) if mode == "signs" else (lambda: -np.ones(n))
    cols = [rng.uniform(-np.pi, np.pi, n) for _ in range(3)]
    cols += [rng.uniform(lo, np.pi - lo, n) * sign() for _ in range(3)]
    cols += [(m + 0.03 * rng.standard_normal(n)) * (rng.choice([-1.0, 1.0], n) if mode == "signs" else 1.0) for m in (1.33, 1.46, 1.52)]
    return np.stack(cols[:F], axis=1).astype(np.float32)


def reparametrise(x, rows) -> np.ndarray:
    """float32 [n, F >= 6] in the column order of NAMES9 with the three bond angles of ``rows`` negated and the torsion each
    one shares an atom with moved by pi and wrapped: the same chain up to the float32 rounding of the torsion.  tau (N:CA:C
    of row i) places the C atom with phi of row i + 1; CA:C:1N goes with psi and C:1N:1CA with omega of the same row.  The last
    row's angles are negated all the same (NeRF does not read them)."""
    x = np.array(x, dtype=np.float32)
    n = len(x)
    wrap = lambda v: (v - 2.0 * np.pi * np.floor((v + np.pi) / (2.0 * np.pi))).astype(np.float32)   # noqa: E731
    for i in np.nonzero(np.asarray(rows, dtype=bool))[0]:
        for ca, ct in ((3, 0), (4, 1), (5, 2)):
            up = 1 if ca == 3 else 0
            x[i, ca] = -x[i, ca]
            if i + up < n:
                x[i + up, ct] = wrap(np.float64(x[i + up, ct]) + np.pi)
    return x


# ---------------------------------------------------------------------------------- 1. the formula against autograd
@pytest.mark.parametrize("F", [3, 6, 9])
@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("n", [2, 3, 7, 40, 128, 600])
def test_vjp_formula_agrees_with_autograd_on_the_whole_domain(F, centered, n):
    """domain_features (bond angles of either sign on both sides of pi / 2, |sin| >= 0.02, lengths of either sign), 2 to 600
    residues: the statement with the forward's rows is within 1e-12 of autograd's largest entry on the float64 restatement's
    own coordinates and within 1e-5 on ref_nerf.build's (float32 products inside); the gates of the backbone-like test below.
    Without the rows (every sign +1) the statement is wrong by about the largest entry itself wherever a sign is negative.

    Measured: on ref_nerf.build's coordinates at most 9.3e-7; on the restatement's own at most 3.9e-14 up to 128 residues and
    7.5e-14 at 600.  (With the restatement's frames recomputed from positions, as ref_nerf.place does, one 600-residue case
    stood at 1.55e-12 -- autograd's own rounding, 1.6e-12 from a long-double evaluation; tests/guide_reference.py carries the
    frame instead and its autograd is within 1.0e-14 of that evaluation.)"""
    idx = IDX[F]
    for m, mode in enumerate(DOMAIN_MODES if n <= 128 else DOMAIN_MODES[:1]):
        rng = np.random.default_rng(100000 * m + 1000 * F + 10 * n + centered)
        ang = domain_features(rng, n, F, mode)
        g = rng.standard_normal((3 * n, 3))
        xyz64, want = gr.autograd_vjp(ang, idx, g, bool(centered))
        xyz32 = gr.build_ref(ang, idx)
        if centered:
            xyz32 = xyz32 - xyz32.mean(axis=0)
        scale = np.abs(want).max()
        on_ref = np.abs(gr.nerf_vjp(xyz32, g, idx, F, centered, ang) - want).max() / scale
        on_own = np.abs(gr.nerf_vjp(xyz64, g, idx, F, centered, ang) - want).max() / scale
        unsigned = np.abs(gr.nerf_vjp(xyz64, g, idx, F, centered) - want).max() / scale
        print(f"F={F} centered={centered} len={n} {mode}: {on_ref:.2e} on ref_nerf's coordinates, {on_own:.2e} on the restatement's, "
              f"{unsigned:.2e} without the rows")
        assert on_ref <= 1e-5 and on_own <= 1e-12
        assert (want[0, 0] == 0) and (want[-1, 1:] == 0).all()
        if F > 3 and mode != "backbone" and n >= 7:
            assert unsigned > 0.1                                       # (the inputs do tell the two statements apart)


def test_reparametrised_rows_build_the_same_chain_and_flip_the_angle_gradient():
    """(angle, torsion) -> (-angle, wrap(torsion + pi)) on a random half of the rows moves no atom by more than 1e-4 A (the
    float32 rounding of the torsion) and negates the angle entries of the gradient exactly in those rows."""
    rng = np.random.default_rng(77)
    n = 24
    ang = random_features(rng, n, 6)
    rows = rng.random(n) < 0.5
    assert rows[:-1].any() and not rows[:-1].all()
    flipped = reparametrise(ang, rows)
    assert (flipped[rows, 3:] < 0).all() and (flipped[~rows, 3:] > 0).all()
    g = rng.standard_normal((3 * n, 3))
    xyz, xyz_f = gr.build_ref(ang, IDX[6]), gr.build_ref(flipped, IDX[6])
    assert np.abs(xyz - xyz_f).max() <= 1e-4
    G, Gf = gr.nerf_vjp(xyz, g, IDX[6], 6, 0, ang), gr.nerf_vjp(xyz_f, g, IDX[6], 6, 0, flipped)
    sign = np.where(rows, -1.0, 1.0)[:, None]
    big = np.abs(G[:, 3:]) > 1e-3 * np.abs(G).max()
    assert big.sum() > n and (np.abs(Gf[:, 3:] - sign * G[:, 3:])[big] <= 1e-4 * np.abs(G[:, 3:])[big]).all()
    assert (np.abs(Gf[:, :3] - G[:, :3]) <= 1e-4 * np.abs(G).max()).all()   # the torsions' entries stay


@pytest.mark.parametrize("F", [3, 6, 9])
@pytest.mark.parametrize("centered", [0, 1])
def test_vjp_formula_agrees_with_autograd(F, centered):
    """On ref_nerf.build's coordinates (float32 cos / sin products inside) the statement is within 1e-5 of the largest
    gradient entry of autograd through the float64 restatement on the same float32 angles -- the float32 products move the
    gradient by 5.5e-7 at 128 residues --, and on the restatement's own coordinates within 1e-12 (1.5e-14 measured)."""
    idx = IDX[F]
    for n in (2, 3, 7, 40, 128):
        rng = np.random.default_rng(1000 * F + 10 * n + centered)
        ang = random_features(rng, n, F)
        g = rng.standard_normal((3 * n, 3))
        xyz64, want = gr.autograd_vjp(ang, idx, g, bool(centered))
        xyz32 = gr.build_ref(ang, idx)
        if centered:
            xyz32 = xyz32 - xyz32.mean(axis=0)
        scale = np.abs(want).max()
        on_ref = np.abs(gr.nerf_vjp(xyz32, g, idx, F, centered) - want).max() / scale
        on_own = np.abs(gr.nerf_vjp(xyz64, g, idx, F, centered) - want).max() / scale
        print(f"F={F} centered={centered} len={n}: {on_ref:.2e} on ref_nerf's coordinates, {on_own:.2e} on the restatement's")
        assert on_ref <= 1e-5 and on_own <= 1e-12
        assert (want[0, 0] == 0) and (want[-1, 1:] == 0).all()          # phi of residue 0, the last residue's other features


# ---------------------------------------------------------------------------------- 2. the builders
def test_contact_and_motif_restraints_and_their_packed_layout():
    c = structures.contact_restraints([(1, 7), (3, 9, 6.5)], max_dist=8.0, weight=2.0)
    assert c.i.tolist() == [4, 10] and c.j.tolist() == [22, 28] and c.d0.tolist() == [0, 0] and c.tol.tolist() == [8.0, 6.5]
    assert c.w.tolist() == [2.0, 2.0] and c.i.dtype == np.int32 and c.d0.dtype == np.float64 and c.min_length() == 10
    assert structures.contact_restraints([(0, 2)], atom="C").i.tolist() == [2]
    rng = np.random.default_rng(3)
    motif = rng.standard_normal((9, 3)) * 4                               # three residues
    m = structures.motif_restraints(motif, [4, 11, 6], weight=0.5, tol=0.25)
    assert list(zip(m.i.tolist(), m.j.tolist())) == [(13, 34), (13, 19), (34, 19)]
    assert np.allclose(m.d0, [np.linalg.norm(motif[1] - motif[4]), np.linalg.norm(motif[1] - motif[7]), np.linalg.norm(motif[4] - motif[7])], rtol=1e-15)
    assert (m.tol == 0.25).all() and (m.w == 0.5).all() and m.min_length() == 12
    both = structures.motif_restraints(motif, [4, 11, 6], atoms=("N", "C"))
    assert len(both) == 15 and (both.i[0], both.j[0]) == (12, 14) and both.d0[0] == np.linalg.norm(motif[0] - motif[2])
    offs, i, j, d0, tol, w = structures.pack_restraints([c, None, m + c], [10, 3, 12])
    assert offs.tolist() == [0, 2, 2, 7] and offs.dtype == np.int32 and i.dtype == np.int32 and w.dtype == np.float64
    assert i.tolist() == [4, 10, 13, 13, 34, 4, 10] and j.tolist() == [22, 28, 34, 19, 19, 22, 28] and tol[2:5].tolist() == [0.25] * 3
    offs, i, *_ = structures.pack_restraints(c, [10, 12])                 # one set for every chain
    assert offs.tolist() == [0, 2, 4] and i.tolist() == [4, 10, 4, 10]
    offs, i, *_ = structures.pack_restraints(None, [5])
    assert offs.tolist() == [0, 0] and len(i) == 0
    for bad in (lambda: structures.contact_restraints([(1, 1)]), lambda: structures.contact_restraints([(-1, 2)]),
                lambda: structures.contact_restraints([(1, 2, 3, 4)]), lambda: structures.contact_restraints([(1, 2)], atom="O"),
                lambda: structures.contact_restraints([(1, 2)], max_dist=-1.0), lambda: structures.contact_restraints([(1, 2)], weight=np.nan),
                lambda: structures.motif_restraints(motif, [4, 11]), lambda: structures.motif_restraints(motif, [4, 4, 6]),
                lambda: structures.motif_restraints(motif, [4, 11, 6], atoms=("CB",)), lambda: structures.motif_restraints(motif, [4, 11, 6], tol=-0.1),
                lambda: structures.motif_restraints(motif * np.inf, [4, 11, 6]),
                lambda: structures.Restraints([1], [1], [0.0], [0.0], [1.0]), lambda: structures.Restraints([1, 2], [3], 1.0, 0.0, 1.0),
                lambda: structures.pack_restraints(c, [10, 9]), lambda: structures.pack_restraints([c], [10, 10])):
        with pytest.raises(ValueError):
            bad()


def test_model_free_entries_reject_bad_arguments_before_touching_a_device(lib):
    """fd_nerf_vjp, fd_restraint_energy and fd_guide_step: every rejection of include/fdmi.h returns -1 with its word in
    fd_last_error() and leaves the outputs alone, on a machine without a GPU too.  No valid call is made."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    f64 = lambda *v: np.array(v, np.float64)                            # noqa: E731
    B, L, F = 2, 6, 6
    lens, idx = i32(4, 6), IDX[6]
    xyz = np.random.default_rng(1).standard_normal((B, 3 * L, 3))
    nan_xyz, inf_g = xyz.copy(), xyz.copy()
    nan_xyz[1, 17, 2], inf_g[0, 11, 0] = np.nan, np.inf                  # the last atoms below the lengths
    pad_nan = xyz.copy()
    pad_nan[0, 12:] = np.nan                                              # beyond chain 0's length: not looked at
    rst = dict(offs=i32(0, 1, 3), ri=i32(1, 4, 0), rj=i32(10, 16, 17), d0=f64(5, 6, 7), tol=f64(0, 1, 0), w=f64(1, 0, 2))
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    def vjp(coords=xyz, lens=lens, B=B, F=F, idx=idx, g=xyz, out="default"):
        out = np.full((2, L, 16), -7.0) if isinstance(out, str) else out
        return [out], lib.fd_nerf_vjp(0, P(coords), P(lens), B, L, F, P(idx), 1, P(g), P(out))

    shape_cases = [(dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"), (dict(B=0), b"B=0"),
                   (dict(F=2), b"F=2 outside [3, 16]"), (dict(F=17), b"F=17 outside [3, 16]"),
                   (dict(idx=i32(0, 1, 6, 3, 4, 5, -1, -1, -1)), b"feat_idx[2]=6"), (dict(idx=i32(0, -1, 2, 3, 4, 5, -1, -1, -1)), b"feat_idx[1]=-1"),
                   (dict(idx=i32(0, 1, 2, 3, 4, 5, -2, -1, -1)), b"feat_idx[6]=-2"), (dict(idx=i32(0, 1, 2, 3, 3, 5, -1, -1, -1)), b"feat_idx[4]=3 repeats")]
    for kw, word in [(dict(coords=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(g=None), b"null"),
                     (dict(out=None), b"null"), (dict(coords=nan_xyz), b"coords is not finite at chain 1, atom 17"),
                     (dict(g=inf_g), b"dcoords is not finite at chain 0, atom 11")] + shape_cases:
        expect(word, *vjp(**kw))
    assert vjp(coords=pad_nan, lens=i32(4, 0))[1] == -1 and b"lens" in lib.fd_last_error()   # (a length error, not the padding's NaN)

    def energy(coords=xyz, lens=lens, B=B, e="default", grad="default", **r):
        a = dict(rst, **r)
        e = np.full(2, -7.0) if isinstance(e, str) else e
        mv, grad = np.full(2, -7.0), (np.full((2, 3 * L, 3), -7.0) if isinstance(grad, str) else grad)
        return [e, mv, grad], lib.fd_restraint_energy(0, P(coords), P(lens), B, L, P(a["offs"]), P(a["ri"]), P(a["rj"]), P(a["d0"]), P(a["tol"]),
                                                      P(a["w"]), P(e), P(mv), P(grad))

    rst_cases = [(dict(offs=None), b"rst_offsets"), (dict(offs=i32(1, 1, 3)), b"rst_offsets[0]=1"), (dict(offs=i32(0, 2, 1)), b"rst_offsets[2]=1 is below"),
                 (dict(ri=None), b"restraint lists"), (dict(w=None), b"restraint lists"),
                 (dict(ri=i32(12, 4, 0)), b"restraint 0 = atoms (12, 10) outside chain 0's [0, 12)"), (dict(rj=i32(10, 16, 18)), b"restraint 2 = atoms (0, 18) outside chain 1"),
                 (dict(ri=i32(-1, 4, 0)), b"restraint 0"), (dict(rj=i32(10, 4, 17)), b"restraint 1 names atom 4 twice"),
                 (dict(d0=f64(5, -1, 7)), b"restraint 1: d0"), (dict(d0=f64(5, 6, np.inf)), b"restraint 2: d0"), (dict(tol=f64(0, 1, -0.5)), b"restraint 2: tol"),
                 (dict(tol=f64(np.nan, 1, 0)), b"restraint 0: tol"), (dict(w=f64(-1, 0, 2)), b"restraint 0: w"), (dict(w=f64(1, np.inf, 2)), b"restraint 1: w")]
    for kw, word in [(dict(coords=None), b"null"), (dict(lens=None), b"null"), (dict(e=None), b"null"), (dict(B=0), b"B=0"),
                     (dict(lens=i32(4, 7)), b"outside [1, 6]"), (dict(coords=nan_xyz), b"coords is not finite")] + rst_cases:
        expect(word, *energy(**kw))

    x = np.random.default_rng(2).standard_normal((B, L, F)).astype(np.float32)
    nan_x = x.copy()
    nan_x[0, 3, 5] = np.nan
    ang, off = np.ones(F, np.uint8), np.zeros(F, np.float32)
    bad_off = off.copy()
    bad_off[2] = np.inf

    def step(x=x, x0=x, lens=lens, B=B, F=F, idx=idx, offset=off, ang=ang, c=0.1, max_norm=1.0, s=0.0, out="default", **r):
        a = dict(rst, **r)
        out = np.full((2, L, 16), -7, np.float32) if isinstance(out, str) else out
        e, gn = np.full(2, -7.0), np.full(2, -7.0)
        return [out, e, gn], lib.fd_guide_step(0, P(x), P(x0), P(lens), B, L, F, P(idx), P(offset), P(ang), P(a["offs"]), P(a["ri"]), P(a["rj"]),
                                               P(a["d0"]), P(a["tol"]), P(a["w"]), C.c_float(c), C.c_double(max_norm), C.c_float(s), None,
                                               C.c_uint64(1), 0, C.c_int64(0), P(out), P(e), P(gn))

    for kw, word in [(dict(x=None), b"null"), (dict(x0=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(ang=None), b"null"),
                     (dict(out=None), b"null"), (dict(c=np.nan), b"c = "), (dict(s=np.inf), b"s = inf"), (dict(max_norm=0.0), b"max_norm=0"),
                     (dict(max_norm=-1.0), b"max_norm=-1"), (dict(max_norm=np.nan), b"max_norm="), (dict(offset=bad_off), b"offset[2]"),
                     (dict(x=nan_x), b"x is not finite at sequence 0, position 3"), (dict(x0=nan_x), b"x0 is not finite")] + shape_cases + rst_cases:
        expect(word, *step(**kw))
    assert checked == (7 + 9) + (6 + 15) + (14 + 9 + 15)


def test_nerf_vjp_feats_is_additive_and_rejects_what_fd_nerf_vjp_rejects(lib):
    """The ABI stays at 7; fd_nerf_vjp_feats has fd_nerf_vjp's rejections plus a null or non-finite `feats` on the rows below a
    length.  No valid call is made."""
    import os
    import re
    from conftest import REPO
    from foldingdiff_amd import _binding
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert "#define FDMI_ABI_VERSION 7" in header and lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7
    assert hasattr(lib, "fd_nerf_vjp_feats") and re.search(r"\bint fd_nerf_vjp_feats\(", header) and re.search(r"\bint fd_nerf_vjp\(", header)
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    B, L, F = 2, 6, 6
    lens, idx = i32(4, 6), IDX[6]
    rng = np.random.default_rng(1)
    xyz = rng.standard_normal((B, 3 * L, 3))
    rows = rng.standard_normal((B, L, F)).astype(np.float32)
    nan_xyz, inf_g, nan_rows, pad_nan = xyz.copy(), xyz.copy(), rows.copy(), rows.copy()
    nan_xyz[1, 17, 2], inf_g[0, 11, 0], nan_rows[0, 3, 4] = np.nan, np.inf, np.nan
    pad_nan[0, 4:] = np.nan                                               # beyond chain 0's length: not looked at

    def call(coords=xyz, lens=lens, B=B, F=F, idx=idx, g=xyz, feats=rows, out="default"):
        out = np.full((2, L, 16), -7.0) if isinstance(out, str) else out
        return out, lib.fd_nerf_vjp_feats(0, P(coords), P(lens), B, L, F, P(idx), 1, P(g), P(feats), P(out))

    cases = [(dict(coords=None), b"null"), (dict(lens=None), b"null"), (dict(idx=None), b"null"), (dict(g=None), b"null"), (dict(feats=None), b"null"),
             (dict(out=None), b"null"), (dict(coords=nan_xyz), b"coords is not finite at chain 1, atom 17"),
             (dict(g=inf_g), b"dcoords is not finite at chain 0, atom 11"), (dict(feats=nan_rows), b"feats is not finite at sequence 0, position 3"),
             (dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"), (dict(B=0), b"B=0"), (dict(F=2), b"F=2 outside [3, 16]"),
             (dict(F=17), b"F=17 outside [3, 16]"), (dict(idx=i32(0, 1, 6, 3, 4, 5, -1, -1, -1)), b"feat_idx[2]=6"),
             (dict(idx=i32(0, 1, 2, 3, 3, 5, -1, -1, -1)), b"feat_idx[4]=3 repeats")]
    for kw, word in cases:
        out, rc = call(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert out is None or (out == -7).all(), word
    assert call(feats=pad_nan, lens=i32(4, 0))[1] == -1 and b"lens" in lib.fd_last_error()   # (a length error, not the padding's NaN)


# ---------------------------------------------------------------------------------- 3. the coefficients
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_guidance_coefficients_against_their_formula(schedule):
    T = 50
    betas = beta_schedules.get_variance_schedule(schedule, T)
    visits = sampling.ddim_visits(T, 9)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    acp = np.concatenate([[1.0], np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))])
    want = 0.7 * (-coef[1].astype(np.float64)) * np.sqrt(1.0 - acp[np.asarray(visits) + 1])
    got = sampling.guidance_coefficients(betas, visits, coef, 0.7)
    assert got.dtype == np.float32 and got.shape == (9,) and np.array_equal(got, want.astype(np.float32))
    assert (got > 0).all()                                                 # b < 0 at every visit: a step DOWN the gradient
    late = sampling.guidance_coefficients(betas, visits, coef, 0.7, guide_from=20)
    assert np.array_equal(late[visits > 20], np.zeros((visits > 20).sum(), np.float32)) and np.array_equal(late[visits <= 20], got[visits <= 20])
    assert (visits > 20).any() and (visits <= 20).any()
    assert not sampling.guidance_coefficients(betas, visits, coef, 0.0).any()
    for bad in (dict(scale=np.inf), dict(coef=coef[:, :5]), dict(visits=[50, 3])):
        kw = dict(dict(betas=betas, visits=visits, coef=coef, scale=1.0), **bad)
        with pytest.raises(ValueError):
            sampling.guidance_coefficients(**kw)


# ---------------------------------------------------------------------------------- 4. descent with the reference alone
def descent_case(seed):
    """A 24-residue chain of six angle features and, as restraints, the 28 CA-CA distances among MOTIF_RES in another chain."""
    rng = np.random.default_rng(seed)
    x = random_features(rng, 24, 6)[None]
    target = gr.build_ref(random_features(rng, 24, 6), IDX[6])
    ca = [3 * r + 1 for r in MOTIF_RES]
    pairs = [(a, b) for k, a in enumerate(ca) for b in ca[k + 1:]]
    rst = ([p[0] for p in pairs], [p[1] for p in pairs], [float(np.linalg.norm(target[a] - target[b])) for a, b in pairs], [0.0] * 28, [1.0] * 28)
    return x, rst


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fifty_guide_statements_bring_the_energy_to_a_quarter(seed):
    """x0 = x, c = 0.05, max_norm = 1, s = 0: the first step lowers the energy and after 50 it is at most a quarter of the
    start.  (Not monotone at a fixed step, so nothing is asked in between.)"""
    x, rst = descent_case(seed)
    energies = []
    for _ in range(50):
        x, e, _, _ = gr.guide_step(x, x, [24], IDX[6], None, [True] * 6, [rst], 0.05, 1.0)
        energies.append(e[0])
    final = gr.restraint_energy(gr.build_ref(x[0], IDX[6]), rst)[0]
    print(f"seed {seed}: energy {energies[0]:.2f} -> {energies[1]:.2f} -> ... -> {final:.2f} (a factor of {energies[0] / final:.1f})")
    assert energies[1] < energies[0] and final <= 0.25 * energies[0]
