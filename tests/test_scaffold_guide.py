"""Restraint guidance combined with replacement without a device: the scaffold-guide statement of
tests/scaffold_guide_reference.py against finite differences and against the relax energy's gradient, the segment restraints,
the arrays sampling.scaffold_segments builds, guide_inpaint's host preparation through a recording stand-in, the rejections of
the two new entries (checked on the host before any device call), the header, and a descent that uses the reference alone."""
import ctypes as C
import inspect
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

import guide_reference as gr
import relax_reference as xr
import scaffold_guide_reference as sg
from conftest import REPO
from foldingdiff_amd import _binding, datasets, sampling, structures
from test_guide import IDX, random_features

# two held segments [lo, hi) per chain length; the lead element of a segment is tau (column 3) of the row before it
HELD = {3: ((0, 1), (2, 3)), 7: ((1, 3), (5, 7)), 24: ((3, 9), (15, 21)), 40: ((5, 13), (22, 30))}
CLASH = sg.Clash(0.63, 0.15, 1.0)


def held_mask(n, F=6) -> np.ndarray:
    """bool [n, F]: the rows of HELD[n] and, per segment that does not start the chain, the lead element."""
    fixed = np.zeros((n, F), dtype=bool)
    for lo, hi in HELD[n]:
        fixed[lo:hi] = True
    for lo, _ in HELD[n]:
        if lo >= 1:
            fixed[lo - 1, 3] = True
    return fixed


def between_segments(target_xyz, segs):
    """(i, j, d0, tol, w): the CA-CA pairs across two segments at their distances in ``target_xyz``."""
    a, b = (list(range(lo, hi)) for lo, hi in segs)
    pairs = [(3 * p + 1, 3 * q + 1) for p in a for q in b]
    return ([p[0] for p in pairs], [p[1] for p in pairs], [float(np.linalg.norm(target_xyz[i] - target_xyz[j])) for i, j in pairs],
            [0.0] * len(pairs), [1.0] * len(pairs))


# ---------------------------------------------------------------------------------- 1. the masked gradient
@pytest.mark.parametrize("n", [3, 7, 24, 40])
def test_masked_gradient_agrees_with_finite_differences(n):
    """E_rst + E_clash of the float64 restatement, central differences with h = 1e-6 over the free elements of the six NeRF
    columns, two held segments and a pinned lead element: within 1e-6 of the largest entry.  The truncation error is h^2 times
    a third derivative (1e-12 of an entry), the rounding error eps E / h (about 1e-16 x 1e3 / 1e-6 = 1e-7 absolute against
    entries of 1e2 and more).  Fixed elements are exactly 0."""
    rng = np.random.default_rng(400 + n)
    ang = random_features(rng, n, 6).astype(np.float64)
    target = gr.build_ref(random_features(rng, n, 6), IDX[6])
    rst = between_segments(target, HELD[n])
    fixed = held_mask(n)
    e0, G = sg.energy64(ang, IDX[6], rst, CLASH)
    masked = np.where(fixed, 0.0, G)
    fd = np.zeros_like(G)
    h = 1e-6
    for l, f in zip(*np.nonzero(~fixed)):
        up, down = ang.copy(), ang.copy()
        up[l, f] += h
        down[l, f] -= h
        fd[l, f] = (sg.energy64(up, IDX[6], rst, CLASH)[0] - sg.energy64(down, IDX[6], rst, CLASH)[0]) / (2 * h)
    scale = np.abs(masked).max()
    err = np.abs(masked - fd).max() / scale
    print(f"len={n}: E = {e0:.3f}, largest entry {scale:.3e}, masked G against central differences {err:.2e}")
    assert scale > 0 and err <= 1e-6
    assert (masked[fixed] == 0).all() and fixed[HELD[n][1][0] - 1, 3] and (np.abs(G[fixed]) > 0).any()
    # the statement's own G (float32 rows, as the device reads them) on the same rows: the mask is what the step applies
    x = ang.astype(np.float32)[None]
    _, _, _, _, _, Gs = sg.step(x, x, x, fixed[None], [n], IDX[6], None, [True] * 6, [rst], 0.05, 1.0, clash=CLASH)
    assert (Gs[0][fixed] == 0).all() and np.abs(Gs[0] - masked).max() <= 1e-5 * scale


@pytest.mark.parametrize("F", [3, 6, 9])
def test_unmasked_gradient_is_the_relax_energys(F):
    """Nothing fixed, no tether, every NeRF column movable: the statement's G is relax_reference.relax_energy's gradient on the
    same coordinates -- within 1e-12 of the largest entry, tests/test_relax.py's gate on the restatement's own coordinates (the
    two add the restraints' and the clashes' coordinate gradients in opposite orders, and a + b == b + a: 0 measured)."""
    for n in (3, 7, 24, 40):
        rng = np.random.default_rng(500 + 10 * F + n)
        ang = random_features(rng, n, F)
        target = gr.build_ref(random_features(rng, n, 6), IDX[6])
        rst = between_segments(target, HELD[n])
        named = [f in set(IDX[F].tolist()) for f in range(F)]
        prm = xr.Params(IDX[F], [True] * F, named, alpha=CLASH.alpha, margin=CLASH.margin, w_clash=CLASH.w)
        e_rst, _, e_clash, G, coords = sg.energy(ang, IDX[F], rst, CLASH)
        e3, G_relax, _, _ = xr.relax_energy(ang, None, prm, None, rst, coords=coords)
        err = np.abs(G - G_relax).max() / np.abs(G_relax).max()
        print(f"F={F} len={n}: {err:.2e}")
        assert err <= 1e-12 and e3[0] == e_clash and e3[1] == e_rst and e3[2] == 0


# ---------------------------------------------------------------------------------- 2. the builders
def test_segment_restraints_keep_the_pairs_across_segments_with_motif_restraints_bits():
    rng = np.random.default_rng(8)
    motif = rng.standard_normal((3 * 12, 3)) * 5
    segs = [(1, 4, 10), (6, 8, 30), (9, 12, 20)]
    for atoms in (("CA",), ("N", "C")):
        got = structures.segment_restraints(motif, segs, weight=0.5, tol=0.25, atoms=atoms)
        rows = [1, 2, 3, 6, 7, 9, 10, 11]
        placed = [10, 11, 12, 30, 31, 20, 21, 22]
        every = structures.motif_restraints(motif.reshape(12, 3, 3)[rows].reshape(-1, 3), placed, weight=0.5, tol=0.25, atoms=atoms)
        k = len(atoms)
        within = sum((k * m) * (k * m - 1) // 2 for m in (3, 2, 3))
        assert len(every) == (8 * k) * (8 * k - 1) // 2 and len(got) == len(every) - within
        seg_of = {p: s for s, ps in enumerate(([10, 11, 12], [30, 31], [20, 21, 22])) for p in ps}
        keep = np.array([seg_of[i // 3] != seg_of[j // 3] for i, j in zip(every.i.tolist(), every.j.tolist())])
        assert np.array_equal(got.i, every.i[keep]) and np.array_equal(got.j, every.j[keep])
        assert np.array_equal(got.d0.view(np.uint64), every.d0[keep].view(np.uint64))      # motif_restraints' distances, bit for bit
        assert (got.tol == 0.25).all() and (got.w == 0.5).all() and got.min_length() == 32
    assert len(structures.segment_restraints(motif, [(0, 5, 3)])) == 0                       # one segment: nothing to place
    for bad in (lambda: structures.segment_restraints(motif, [(0, 3, 0), (2, 5, 10)]),       # a shared motif residue
                lambda: structures.segment_restraints(motif, [(0, 3, 0), (5, 8, 2)]),        # a shared placed residue
                lambda: structures.segment_restraints(motif, [(3, 3, 0)]), lambda: structures.segment_restraints(motif, [(10, 13, 0)]),
                lambda: structures.segment_restraints(motif, [(0, 3, -1)]), lambda: structures.segment_restraints(motif, [(0, 3)]),
                lambda: structures.segment_restraints(motif[:-1], [(0, 3, 0)]),
                lambda: structures.segment_restraints(motif, segs, atoms=("CB",)), lambda: structures.segment_restraints(motif, segs, tol=-0.1),
                lambda: structures.segment_restraints(motif * np.inf, segs)):
        with pytest.raises(ValueError):
            bad()


class _Model:
    n_inputs = 6
    device = torch.device("cpu")

    def prepare(self, betas, is_angle=None):
        return 0

    def set_option(self, name, value):
        return 0


def _dset(offset=None, pad=48, T=12):
    return datasets.NoisedAnglesDataset(datasets.AnglesEmptyDataset("canonical-full-angles", pad=pad, mean_offset=offset), timesteps=T,
                                        beta_schedule="cosine")


def _recorded(fn):
    """The arguments of the one runner call ``fn`` makes per batch, with a stand-in that copies x0 into out."""
    calls = []
    sig = inspect.signature(sampling._run_fd_sample_guided_inpaint)

    def stand_in(*args, **kwargs):
        a = dict(sig.bind(*args, **kwargs).arguments)
        calls.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()})
        a["out"][...] = a["x0"]
        a["energy"][:, 0], a["energy"][:, 1], a["worst"][:] = 1.0 + np.arange(len(a["worst"])), 0.5, 2.0
    with mock.patch.object(sampling, "_run_fd_sample_guided_inpaint", stand_in):
        torch.manual_seed(7)
        returned = fn()
    return calls, returned


OFFSET = np.array([0.3, -0.2, 3.0, 1.9, 2.0, 2.1], dtype=np.float32)


def test_scaffold_segments_builds_known_fixed_and_the_restraints():
    rng = np.random.default_rng(9)
    motif_angles = random_features(rng, 12, 6)
    motif_xyz = gr.build_ref(motif_angles, IDX[6])
    segs = [(0, 3, 0), (5, 8, 10), (9, 11, 20)]          # the first at residue 0: no lead element
    ds = _dset(OFFSET)
    calls, (samples, info) = _recorded(lambda: sampling.scaffold_segments(_Model(), ds, motif_angles, motif_xyz, segs, [24, 30], num_steps=4,
                                                                         clash_weight=2.0, max_norm=0.5))
    assert len(calls) == 1 and [s.shape for s in samples] == [(24, 6), (30, 6)]
    c = calls[0]
    fixed, known = c["fixed"], c["known"]
    assert fixed.dtype == np.uint8 and fixed.shape == (2, 30, 6) and known.dtype == np.float32
    want = np.zeros((30, 6), dtype=bool)
    want[0:3], want[10:13], want[20:22] = True, True, True
    want[9, 3], want[19, 3] = True, True                 # tau of the row in front of the second and the third segment
    for b, n in enumerate((24, 30)):
        assert np.array_equal(fixed[b].astype(bool)[:n], want[:n]) and not fixed[b, n:].any()
    model_space = lambda rows: sampling._model_space(rows, OFFSET, np.ones(6, dtype=bool))   # noqa: E731
    assert np.array_equal(known[0, 10:13], model_space(motif_angles[5:8])) and np.array_equal(known[1, 20:22], model_space(motif_angles[9:11]))
    assert known[0, 9, 3] == model_space(motif_angles[4:5])[0, 3] and known[0, 19, 3] == model_space(motif_angles[8:9])[0, 3]   # the motif row before
    assert not known[0][~want].any()
    rst = structures.segment_restraints(motif_xyz, segs)
    offs, ri, rj, d0, tol, w = c["packed"]
    assert offs.tolist() == [0, len(rst), 2 * len(rst)] and np.array_equal(ri[: len(rst)], rst.i) and np.array_equal(d0[len(rst):], rst.d0)
    p = c["params"]
    assert (p.w_clash, p.clash_alpha, p.clash_margin, p.max_norm, p.has_offset) == (2.0, 0.63, 0.15, 0.5, 1)
    assert np.array_equal(info["energy"], [1.0, 2.0]) and np.array_equal(info["clash_energy"], [0.5, 0.5]) and np.array_equal(info["max_violation"], [2.0, 2.0])
    # a segment that starts at motif residue 0 away from the chain start takes its own first tau, as structures.motif_backbone does
    calls, _ = _recorded(lambda: sampling.scaffold_segments(_Model(), ds, motif_angles, motif_xyz, [(0, 3, 4), (5, 8, 10)], [20], num_steps=4))
    assert calls[0]["known"][0, 3, 3] == model_space(motif_angles[0:1])[0, 3] and calls[0]["fixed"][0, 3].tolist() == [0, 0, 0, 1, 0, 0]
    calls, _ = _recorded(lambda: sampling.scaffold_segments(_Model(), ds, motif_angles, motif_xyz, segs, [24], num_steps=4, pin_lead_angle=False))
    assert not calls[0]["fixed"][0, 9].any() and calls[0]["fixed"][0].sum() == 8 * 6
    # adjacent segments: the row in front of the second is held already and keeps its own tau
    calls, _ = _recorded(lambda: sampling.scaffold_segments(_Model(), ds, motif_angles, motif_xyz, [(0, 3, 5), (6, 9, 8)], [20], num_steps=4))
    assert calls[0]["known"][0, 7, 3] == model_space(motif_angles[2:3])[0, 3]
    for bad in (dict(segments=[(0, 3, 0), (2, 5, 10)]), dict(segments=[(0, 3, 0), (5, 8, 2)]), dict(segments=[(0, 3, 22), (5, 8, 10)]),
                dict(segments=[(0, 13, 0)]), dict(motif_backbone=motif_xyz[:-3])):
        kw = dict(dict(segments=segs, motif_backbone=motif_xyz), **bad)
        with pytest.raises(ValueError):
            sampling.scaffold_segments(_Model(), ds, motif_angles, kw["motif_backbone"], kw["segments"], [24], num_steps=4)


def test_guide_inpaint_prepares_the_call():
    rng = np.random.default_rng(10)
    known = [random_features(rng, n, 6) for n in (9, 14, 11)]
    known[1][0, 0] = np.nan                                # free: NaN is allowed there
    fixed = [np.arange(9) % 3 == 1, np.zeros((14, 6), dtype=bool), np.zeros(11, dtype=bool)]
    fixed[1][4, 3], fixed[1][5:8] = True, True
    rst = [structures.contact_restraints([(0, 8)]), None, structures.contact_restraints([(1, 10, 6.0)])]
    ds = _dset(OFFSET, T=12)
    run = lambda **kw: sampling.guide_inpaint(_Model(), ds, known, fixed, rst, **dict(dict(num_steps=5, batch_size=2), **kw))   # noqa: E731
    calls, (samples, info) = _recorded(run)
    assert [c["x0"].shape for c in calls] == [(2, 14, 6), (1, 11, 6)] and [s.shape for s in samples] == [(9, 6), (14, 6), (11, 6)]
    c = calls[0]
    betas = ds.alpha_beta_terms["betas"]
    visits = sampling.ddim_visits(12, 5)
    coef = sampling.steer_coefficients(betas, visits, 1.0)
    assert np.array_equal(c["visits"], visits) and np.array_equal(c["coef"], coef) and c["coef"].shape == (5, 5)
    assert np.array_equal(c["guide_tab"], sampling.guidance_coefficients(betas, visits, coef, 1.0))
    assert np.array_equal(c["known_coef"], sampling.inpaint_levels(betas)) and c["lens"].tolist() == [9, 14]
    assert c["fixed"][0, :9].all(axis=1).tolist() == (np.arange(9) % 3 == 1).tolist() and not c["fixed"][0, 9:].any()
    assert c["fixed"][1].sum() == 1 + 18 and c["fixed"][1, 4].tolist() == [0, 0, 0, 1, 0, 0]
    assert np.isfinite(c["known"]).all() and not c["known"][c["fixed"] == 0].any()
    assert np.array_equal(c["known"][1, 5:8], sampling._model_space(known[1][5:8], OFFSET, np.ones(6, dtype=bool)))
    assert c["packed"][0].tolist() == [0, 1, 1] and calls[1]["packed"][0].tolist() == [0, 1] and calls[1]["packed"][4].tolist() == [6.0]
    assert (c["params"].w_clash, c["params"].max_norm) == (0.0, 1.0) and list(c["params"].feat_idx) == [0, 1, 2, 3, 4, 5, -1, -1, -1]
    assert calls[0]["seed"] != calls[1]["seed"] and sorted(info) == ["clash_energy", "energy", "guide", "max_violation", "visits"]
    assert info["energy"].tolist() == [1.0, 2.0, 1.0]
    # the defaults of the clash term are structures.relax' own
    relax_sig, own = inspect.signature(structures.relax).parameters, inspect.signature(sampling.guide_inpaint).parameters
    assert own["clash_alpha"].default == relax_sig["alpha"].default and own["clash_margin"].default == relax_sig["margin"].default
    assert own["clash_weight"].default == 0.0
    # seed: the same draws from a generator of its own
    a, _ = _recorded(lambda: run(seed=5))
    torch.manual_seed(99)
    b, _ = _recorded(lambda: run(seed=5))
    assert np.array_equal(a[0]["x0"], b[0]["x0"]) and a[0]["seed"] == b[0]["seed"] and not np.array_equal(a[0]["x0"], calls[0]["x0"])
    nan_known = [k.copy() for k in known]
    nan_known[0][1, 2] = np.nan                            # fixed there
    for bad in (dict(max_norm=0.0), dict(clash_weight=-1.0), dict(clash_alpha=np.nan), dict(clash_margin=-0.1), dict(num_steps=0), dict(eta=2.0),
                dict(batch_size=0)):
        with pytest.raises(ValueError):
            run(**bad)
    with pytest.raises(ValueError):
        sampling.guide_inpaint(_Model(), ds, nan_known, fixed, rst, num_steps=5)
    with pytest.raises(ValueError):                        # a restraint beyond its chain
        sampling.guide_inpaint(_Model(), ds, known, fixed, structures.contact_restraints([(0, 12)]), num_steps=5)
    with pytest.raises(ValueError):                        # longer than the dataset pads to
        sampling.guide_inpaint(_Model(), ds, [random_features(rng, 49, 6)], [np.zeros(49, dtype=bool)], None, num_steps=5)


# ---------------------------------------------------------------------------------- 3. the entries
def test_header_abi_and_binding_hold_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert "#define FDMI_ABI_VERSION 7" in header and lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7
    for name in ("fd_scaffold_guide_step", "fd_sample_guided_inpaint"):
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _binding.exported_symbols()
    assert "typedef struct fd_scaffold_guide_params" in header
    fields = [f[0] for f in _binding.FdScaffoldGuideParams._fields_]
    assert fields == ["feat_idx", "has_offset", "offset", "max_norm", "clash_alpha", "clash_margin", "w_clash"]
    assert C.sizeof(_binding.FdScaffoldGuideParams) == C.sizeof(_binding.FdGuideParams) + 24    # additive: fd_guide_params did not grow
    assert C.sizeof(_binding.FdGuideParams) == 9 * 4 + 4 + 16 * 4 + 8


def test_the_step_hook_rejects_bad_arguments_before_touching_a_device(lib):
    """Every rejection of include/fdmi.h returns -1 with its word in fd_last_error() and leaves the outputs alone, on a machine
    without a GPU too.  No valid call is made."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    f64 = lambda *v: np.array(v, np.float64)                            # noqa: E731
    B, L, F = 2, 6, 6
    lens = i32(4, 6)
    rst = dict(offs=i32(0, 1, 3), ri=i32(1, 4, 0), rj=i32(10, 16, 17), d0=f64(5, 6, 7), tol=f64(0, 1, 0), w=f64(1, 0, 2))
    x = np.random.default_rng(2).standard_normal((B, L, F)).astype(np.float32)
    fixed = np.zeros((B, L, F), np.uint8)
    fixed[0, 1], fixed[1, 4, 3] = 1, 1
    nan_x, nan_x0_free, nan_x0_fixed, nan_known, nan_known_free, beyond = x.copy(), x.copy(), x.copy(), x.copy(), x.copy(), fixed.copy()
    nan_x[0, 3, 5], nan_x0_free[1, 2, 0], nan_x0_fixed[0, 1, 2], nan_known[1, 4, 3], nan_known_free[0, 0, 0], beyond[0, 4, 1] = (np.nan,) * 5 + (1,)
    ang = np.ones(F, np.uint8)

    def params(idx=IDX[6], offset=None, max_norm=1.0, alpha=0.63, margin=0.15, w=1.0):
        p = _binding.FdScaffoldGuideParams()
        p.feat_idx[:] = [int(v) for v in idx]
        p.has_offset = 0 if offset is None else 1
        if offset is not None:
            p.offset[:F] = [float(v) for v in offset]
        p.max_norm, p.clash_alpha, p.clash_margin, p.w_clash = max_norm, alpha, margin, w
        return p

    def step(x=x, x0=x, known=x, fixed=fixed, lens=lens, B=B, F=F, ang=ang, prm="default", c=0.1, s=0.0, out="default", e="default", mv="default",
             gn="default", **r):
        a = dict(rst, **r)
        prm = params() if isinstance(prm, str) else prm
        out = np.full((2, L, 16), -7, np.float32) if isinstance(out, str) else out
        e, mv, gn = (np.full(n, -7.0) if isinstance(v, str) else v for v, n in ((e, 4), (mv, 2), (gn, 2)))
        G = np.full((2, L, 16), -7.0)
        rc = lib.fd_scaffold_guide_step(0, P(x), P(x0), P(known), P(fixed), P(lens), B, L, F, P(ang), None if prm is None else C.byref(prm),
                                        P(a["offs"]), P(a["ri"]), P(a["rj"]), P(a["d0"]), P(a["tol"]), P(a["w"]), C.c_float(c), C.c_float(s), None,
                                        C.c_uint64(1), 0, C.c_int64(0), P(out), P(e), P(mv), P(gn), P(G))
        return [out, e, mv, gn, G], rc

    bad_off = np.zeros(F, np.float32)
    bad_off[2] = np.inf
    cases = [(dict(x=None), b"null"), (dict(x0=None), b"null"), (dict(lens=None), b"null"), (dict(ang=None), b"null"), (dict(prm=None), b"null"),
             (dict(out=None), b"null"), (dict(e=None), b"null"), (dict(mv=None), b"null"), (dict(gn=None), b"null"),
             (dict(known=None), b"known is null"), (dict(fixed=None), b"fixed is null"),
             (dict(c=np.nan), b"c = "), (dict(s=np.inf), b"s = inf"),
             (dict(prm=params(max_norm=0.0)), b"max_norm=0"), (dict(prm=params(max_norm=-1.0)), b"max_norm=-1"), (dict(prm=params(max_norm=np.nan)), b"max_norm="),
             (dict(prm=params(offset=bad_off)), b"offset[2]"),
             (dict(prm=params(alpha=-0.1)), b"clash_alpha=-0.1"), (dict(prm=params(alpha=np.inf)), b"clash_alpha=inf"),
             (dict(prm=params(margin=-1.0)), b"clash_margin=-1"), (dict(prm=params(margin=np.nan)), b"clash_margin="),
             (dict(prm=params(w=-2.0)), b"w_clash=-2"), (dict(prm=params(w=np.inf)), b"w_clash=inf"),
             (dict(x=nan_x), b"x is not finite at sequence 0, position 3"), (dict(x0=nan_x0_free), b"x0 is not finite at a free element: sequence 1, position 2"),
             (dict(known=nan_known), b"known is not finite at a fixed element: sequence 1 position 4 feature 3"),
             (dict(fixed=beyond), b"fixed element beyond a length: sequence 0 position 4 feature 1"),
             (dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"), (dict(B=0), b"B=0"), (dict(F=2), b"F=2 outside [3, 16]"),
             (dict(F=17), b"F=17 outside [3, 16]"), (dict(prm=params(idx=i32(0, 1, 6, 3, 4, 5, -1, -1, -1))), b"feat_idx[2]=6"),
             (dict(prm=params(idx=i32(0, -1, 2, 3, 4, 5, -1, -1, -1))), b"feat_idx[1]=-1"), (dict(prm=params(idx=i32(0, 1, 2, 3, 3, 5, -1, -1, -1))), b"feat_idx[4]=3 repeats"),
             (dict(offs=None), b"rst_offsets"), (dict(offs=i32(1, 1, 3)), b"rst_offsets[0]=1"), (dict(ri=None), b"restraint lists"),
             (dict(ri=i32(12, 4, 0)), b"restraint 0 = atoms (12, 10) outside chain 0's [0, 12)"), (dict(rj=i32(10, 4, 17)), b"restraint 1 names atom 4 twice"),
             (dict(d0=f64(5, -1, 7)), b"restraint 1: d0"), (dict(tol=f64(np.nan, 1, 0)), b"restraint 0: tol"), (dict(w=f64(1, np.inf, 2)), b"restraint 1: w")]
    for kw, word in cases:
        outs, rc = step(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
    # what is NOT an error gets past the argument checks: a NaN of x0 under a fixed element, a NaN of known under a free one.  (No
    # valid call is made here: the same arrays with a bad length fail on the length, not on the NaN.)
    for kw in (dict(x0=nan_x0_fixed), dict(known=nan_known_free)):
        outs, rc = step(lens=i32(4, 0), **kw)
        assert rc == -1 and b"lens[1]=0" in lib.fd_last_error()


def test_the_run_entry_rejects_a_null_model_and_the_script_has_the_flags(lib):
    """A model handle needs a device, so the run's other rejections are in tests/test_scaffold_guide_gpu.py; what can be asked
    without one: a null handle is an argument error and nothing is written."""
    P = _binding.ptr
    x = np.zeros((1, 4, 6), np.float32)
    out, e, mv = np.full((1, 4, 6), -7, np.float32), np.full(2, -7.0), np.full(1, -7.0)
    prm = _binding.FdScaffoldGuideParams()
    rc = lib.fd_sample_guided_inpaint(None, P(x), P(np.array([4], np.int32)), 1, 4, P(np.array([3, 0], np.int32)), 2, P(np.zeros((5, 2), np.float32)),
                                      None, P(x), P(np.zeros((1, 4, 6), np.uint8)), P(np.zeros(2 * 11, np.float32)), None, C.c_uint64(1), C.c_int64(0),
                                      P(np.zeros(2, np.float32)), C.byref(prm), P(np.zeros(2, np.int32)), None, None, None, None, None, P(out), P(e), P(mv))
    assert rc == -1 and lib.fd_last_error() and (out == -7).all() and (e == -7).all() and (mv == -7).all()
    import importlib.util
    spec = importlib.util.spec_from_file_location("sample_restrained", os.path.join(REPO, "bin", "sample_restrained.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args(["-m", "x", "-l", "30", "--motif_pdb", "m.pdb", "--motif_residues", "3-6,20-22", "--placed_at", "8,25",
                                          "--hold_motif", "--clash_weight", "1.5"])
    assert args.hold_motif is True and args.clash_weight == 1.5
    plain = mod.build_parser().parse_args(["-m", "x", "-l", "30", "--contacts", "c.txt"])
    assert plain.hold_motif is False and plain.clash_weight is None
    for argv in (["-m", "x", "-l", "30", "--contacts", "c.txt", "--hold_motif"], ["-m", "x", "-l", "30", "--contacts", "c.txt", "--clash_weight", "-1"]):
        with pytest.raises(SystemExit):
            mod.main(argv)


# ---------------------------------------------------------------------------------- 4. descent with the reference alone
DESCENT_SEGMENTS = ((3, 9), (15, 21))     # residues 3-8 and 15-20
# E_start / E_end measured over seeds 0 .. 7: 18.41, 8.39, 26.15, 389.42, 11.78, 26.98, 10.15, 104.26; the gate is half the smallest
DESCENT_GATE = 8.39 / 2


def scaffold_descent_case(seed):
    """A 24-residue chain whose residues 3-8 and 15-20 (and the lead element of each) hold a target chain's angles, random free
    angles, and the 36 CA-CA distances between the two segments in the target as restraints."""
    rng = np.random.default_rng(seed)
    x = random_features(rng, 24, 6)
    target_ang = random_features(rng, 24, 6)
    fixed = np.zeros((24, 6), dtype=bool)
    for lo, hi in DESCENT_SEGMENTS:
        fixed[lo:hi] = True
        fixed[lo - 1, 3] = True
    x = np.where(fixed, target_ang, x)
    rst = between_segments(gr.build_ref(target_ang, IDX[6]), DESCENT_SEGMENTS)
    return x[None], target_ang[None], fixed[None], rst


def scaffold_descent(seed, steps=50):
    x, known, fixed, rst = scaffold_descent_case(seed)
    start = x.copy()
    energies = []
    for _ in range(steps):
        x, e, *_ = sg.step(x, x, known, fixed, [24], IDX[6], None, [True] * 6, [rst], 0.05, 1.0)
        energies.append(e[0, 0])
    final = sg.energy(x[0], IDX[6], rst)[0]
    assert np.array_equal(x.view(np.uint32)[fixed], start.view(np.uint32)[fixed])           # the held elements keep their bits throughout
    return energies[0], final


@pytest.mark.parametrize("seed", range(8))
def test_fifty_scaffold_guide_statements_lower_the_restraint_energy(seed):
    """x0 = x, c = 0.05, max_norm = 1, s = 0, no clash term.  Measured factors E_start / E_end over seeds 0 .. 7 are in DESIGN.md
    6y; the gate is half the smallest of them (the descent is clipped with a fixed step and not monotone, and half leaves room
    for another platform's libm)."""
    first, final = scaffold_descent(seed)
    print(f"seed {seed}: E_rst {first:.2f} -> {final:.2f} (a factor of {first / final:.2f})")
    assert first / final >= DESCENT_GATE
