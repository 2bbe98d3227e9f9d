"""Superposition restraints without a device: the template statement of tests/template_reference.py against
finite differences, on a copy and on a mirror image, a descent that uses the reference alone, the builders, the arrays
sampling.scaffold_segments and guide_inpaint prepare (through recording stand-ins), the rejections of the new entries (checked on
the host before any device call), the header and the script's flags."""
import ctypes as C
import importlib.util
import inspect
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

import guide_reference as gr
import scaffold_guide_reference as sg
import template_reference as tr
from conftest import REPO
from foldingdiff_amd import _binding, sampling, structures
from test_guide import IDX, random_features
from test_scaffold_guide import DESCENT_SEGMENTS, OFFSET, _dset, _Model, scaffold_descent_case


def moved(rng, xyz, shift=100.0):
    """A rotated copy of ``xyz`` shifted by ``shift`` Angstrom along a random direction."""
    d = rng.standard_normal(3)
    return xyz @ tr.random_rotation(rng).T + shift * d / np.linalg.norm(d)


# ---------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("n", [3, 7, 24, 40])
def test_gradient_agrees_with_finite_differences(n):
    """E_tpl of the float64 restatement pushed through gr.nerf_vjp against central differences of sg.nerf_scan64 with h = 1e-6
    over the six NeRF columns: a random subset of atoms, weights in [0.5, 2], the target another chain's atoms rotated and
    shifted.  Gate 1e-6 of the largest entry, tests/test_scaffold_guide.py's with its derivation (truncation h^2 times a third
    derivative, rounding eps E / h).  Measured: 7.3e-10, 8.0e-10, 1.9e-9, 7.5e-9."""
    rng = np.random.default_rng(600 + n)
    ang = random_features(rng, n, 6).astype(np.float64)
    target = moved(rng, gr.build_ref(random_features(rng, n, 6), IDX[6]), 30.0)
    atoms = np.sort(rng.choice(3 * n, size=max(4, (3 * n) // 2), replace=False))
    tpl = (atoms, target[atoms], rng.uniform(0.5, 2.0, len(atoms)))
    e0, G = tr.energy64(ang, IDX[6], tpl)
    fd = np.zeros_like(G)
    h = 1e-6
    for l in range(n):
        for f in range(6):
            up, down = ang.copy(), ang.copy()
            up[l, f] += h
            down[l, f] -= h
            fd[l, f] = (tr.energy64(up, IDX[6], tpl)[0] - tr.energy64(down, IDX[6], tpl)[0]) / (2 * h)
    scale = np.abs(G).max()
    err = np.abs(G - fd).max() / scale
    print(f"len={n}: E = {e0:.3f}, {len(atoms)} atoms, largest entry {scale:.3e}, G against central differences {err:.2e}")
    assert scale > 0 and err <= 1e-6


@pytest.mark.parametrize("n", [3, 7, 24, 40])
def test_a_rotated_and_translated_copy_costs_nothing(n):
    """The chain's own atoms, rotated and shifted 100 A, as the template: rmsd <= 1e-12 A and a gradient <= 1e-12 (measured
    at most 3.9e-14 and 1.5e-13), the explicit residuals' doing: lambda_max minus the two norms would leave 1e-6."""
    rng = np.random.default_rng(n)
    xyz = gr.build_ref(random_features(rng, n, 6), IDX[6])
    fit = tr.template_energy(xyz, (np.arange(3 * n), moved(rng, xyz), rng.uniform(0.5, 2.0, 3 * n)))
    print(f"len={n}: rmsd {fit.rmsd:.2e}, largest gradient entry {np.abs(fit.grad).max():.2e}")
    assert fit.rmsd <= 1e-12 and np.abs(fit.grad).max() <= 1e-12
    assert np.abs(fit.R @ fit.R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(fit.R) - 1) <= 1e-12


@pytest.mark.parametrize("n", [7, 24, 40])
def test_a_mirror_image_keeps_every_distance_and_does_not_fit(n):
    """The backbone of default_rng(n) and its reflection z -> -z: an all-pairs distance restraint energy (targets 0.5 A off, so
    that it is not 0) is the same to the bit, the all-atom template of the structure fits the mirror image at >= 1 A
    (measured 2.04, 3.48, 3.71), and the mirrored template fits it exactly."""
    xyz = gr.build_ref(random_features(np.random.default_rng(n), n, 6), IDX[6])
    flipped = xyz * np.array([1.0, 1.0, -1.0])
    i, j = np.triu_indices(3 * n, 1)
    rst = (i, j, np.linalg.norm(xyz[i] - xyz[j], axis=1) + 0.5, np.zeros(len(i)), np.ones(len(i)))
    e, _, _ = gr.restraint_energy(xyz, rst)
    e_flipped, _, _ = gr.restraint_energy(flipped, rst)
    tpl = (np.arange(3 * n), xyz, np.ones(3 * n))
    fit, own = tr.template_energy(flipped, tpl), tr.template_energy(flipped, tr.mirrored(tpl))
    print(f"len={n}: E_rst {e:.3f} both ways, the mirror image fits at {fit.rmsd:.2f} A, its own template at {own.rmsd:.1e}")
    assert e > 0 and e == e_flipped
    assert fit.rmsd >= 1.0 and own.rmsd <= 1e-12 and tr.template_energy(xyz, tpl).rmsd <= 1e-12


# ---------------------------------------------------------------------------------- 2. descent with the reference alone
# E_start / E_end measured over seeds 0 .. 7 with this reference: see the test; the gate is half the smallest
DESCENT_FACTORS = (465.17, 12.21, 144.82, 381.08, 44.58, 92.96, 91.39, 311.64)
DESCENT_GATE = min(DESCENT_FACTORS) / 2


def template_descent_case(seed):
    """tests/test_scaffold_guide.py's descent case with a CA-only template of the 12 held residues, weights 1, in place of
    the 36 distances."""
    x, known, fixed, _ = scaffold_descent_case(seed)
    target = gr.build_ref(known[0], IDX[6])
    atoms = np.array([3 * r + 1 for lo, hi in DESCENT_SEGMENTS for r in range(lo, hi)])
    return x, known, fixed, (atoms, target[atoms], np.ones(len(atoms)))


@pytest.mark.parametrize("seed", range(8))
def test_fifty_statements_lower_the_template_energy(seed):
    """x0 = x, c = 0.05, max_norm = 1, s = 0, no other term.  The gate is half the smallest measured factor, as in DESIGN.md 6y
    (the descent is clipped with a fixed step and not monotone, and half leaves room for another platform's libm); the held
    elements keep their bits."""
    x, known, fixed, tpl = template_descent_case(seed)
    start = x.copy()
    first = None
    for _ in range(50):
        x, e, _, _, rmsd, _ = tr.step(x, x, known, fixed, [24], IDX[6], None, [True] * 6, [None], [tpl], 0.05, 1.0)
        first = (e[0, 2], rmsd[0]) if first is None else first
    final = tr.energy(x[0], IDX[6], None, tpl)
    print(f"seed {seed}: E_tpl {first[0]:.2f} -> {final[3]:.4f} (a factor of {first[0] / final[3]:.2f}), CA rmsd {first[1]:.2f} -> {final[4]:.2f} A")
    assert np.array_equal(x.view(np.uint32)[fixed], start.view(np.uint32)[fixed])
    assert first[0] / final[3] >= DESCENT_GATE


# ---------------------------------------------------------------------------------- 3. the builders
def test_motif_template_and_its_packed_layout():
    rng = np.random.default_rng(8)
    motif = rng.standard_normal((3 * 12, 3)) * 5
    segs = [(6, 8, 30), (1, 4, 10), (9, 12, 20)]               # not in chain order: the template sorts by atom
    t = structures.motif_template(motif, segs, weight=0.5)
    rows, placed = [1, 2, 3, 9, 10, 11, 6, 7], [10, 11, 12, 20, 21, 22, 30, 31]
    assert len(t) == 24 and t.atoms.dtype == np.int32 and t.atoms.tolist() == [3 * p + a for p in placed for a in range(3)]
    assert np.array_equal(t.xyz.view(np.uint64), motif.reshape(12, 3, 3)[rows].reshape(-1, 3).view(np.uint64))   # the motif's bits
    assert (t.w == 0.5).all() and t.min_length() == 32
    ca = structures.motif_template(motif, segs, atoms=("CA",))
    assert ca.atoms.tolist() == [3 * p + 1 for p in placed] and np.array_equal(ca.xyz, motif.reshape(12, 3, 3)[rows, 1]) and (ca.w == 1).all()
    nc = structures.motif_template(motif, segs, atoms=("C", "N"))
    assert nc.atoms.tolist() == [3 * p + a for p in placed for a in (0, 2)]
    assert np.array_equal(t.mirrored().xyz, t.xyz * [1, 1, -1]) and np.array_equal(t.mirrored().atoms, t.atoms)
    for bad in (lambda: structures.motif_template(motif, [(0, 3, 0), (2, 5, 10)]), lambda: structures.motif_template(motif, [(0, 3, 0), (5, 8, 2)]),
                lambda: structures.motif_template(motif, [(3, 3, 0)]), lambda: structures.motif_template(motif, [(10, 13, 0)]),
                lambda: structures.motif_template(motif, [(0, 3, -1)]), lambda: structures.motif_template(motif, [(0, 3)]),
                lambda: structures.motif_template(motif[:-1], [(0, 3, 0)]), lambda: structures.motif_template(motif, segs, atoms=("CB",)),
                lambda: structures.motif_template(motif, segs, weight=0.0), lambda: structures.motif_template(motif * np.inf, segs),
                lambda: structures.Template([1, 1], np.zeros((2, 3))), lambda: structures.Template([-1], np.zeros((1, 3))),
                lambda: structures.Template([1, 2], np.zeros((1, 3))), lambda: structures.Template([1], np.zeros((1, 3)), np.nan)):
        with pytest.raises(ValueError):
            bad()
    offs, atom, xyz, w = structures.pack_templates([t, None, ca], [32, 5, 40])
    assert offs.dtype == np.int32 and offs.tolist() == [0, 24, 24, 32] and atom.dtype == np.int32 and xyz.shape == (32, 3) and w.dtype == np.float64
    assert np.array_equal(atom[:24], t.atoms) and np.array_equal(atom[24:], ca.atoms) and np.array_equal(xyz[24:], ca.xyz) and w.tolist() == [0.5] * 24 + [1.0] * 8
    assert structures.pack_templates(ca, [32, 33])[0].tolist() == [0, 8, 16] and structures.pack_templates(None, [4])[0].tolist() == [0, 0]
    for bad in (lambda: structures.pack_templates(t, [31]), lambda: structures.pack_templates([t], [32, 32])):
        with pytest.raises(ValueError):
            bad()


def _recorded(fn):
    """The arguments of every runner call ``fn`` makes, plain or with templates, with stand-ins that copy x0 into out."""
    calls = []
    plain, with_tpl = inspect.signature(sampling._run_fd_sample_guided_inpaint), inspect.signature(sampling._run_fd_sample_guided_inpaint_tpl)

    def stand_in(sig, name):
        def run(*args, **kwargs):
            a = dict(sig.bind(*args, **kwargs).arguments)
            calls.append(dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}, runner=name))
            a["out"][...] = a["x0"]
            a["energy"][:, 0], a["energy"][:, 1], a["worst"][:] = 1.0 + np.arange(len(a["worst"])), 0.5, 2.0
            if name == "tpl":
                a["energy"][:, 2], a["tpl_rmsd"][:] = 7.0, 0.25
        return run
    with mock.patch.object(sampling, "_run_fd_sample_guided_inpaint", stand_in(plain, "plain")), \
            mock.patch.object(sampling, "_run_fd_sample_guided_inpaint_tpl", stand_in(with_tpl, "tpl")):
        torch.manual_seed(7)
        returned = fn()
    return calls, returned


def test_scaffold_segments_places_by_distances_template_or_both():
    rng = np.random.default_rng(9)
    motif_angles = random_features(rng, 12, 6)
    motif_xyz = gr.build_ref(motif_angles, IDX[6])
    segs = [(0, 3, 0), (5, 8, 10), (9, 11, 20)]
    ds = _dset(OFFSET)
    run = lambda **kw: _recorded(lambda: sampling.scaffold_segments(_Model(), ds, motif_angles, motif_xyz, segs, [24, 30], num_steps=4, **kw))   # noqa: E731
    rst = structures.segment_restraints(motif_xyz, segs)
    extra = structures.contact_restraints([(1, 15)])
    # the default makes the call it made before the term existed: the plain runner, [B, 2] energies, five info keys
    (default,), (_, info) = run()
    (named,), _ = run(placement="distances")
    assert default["runner"] == named["runner"] == "plain" and default["energy"].shape == (2, 2) and "tpl_packed" not in default
    assert sorted(info) == ["clash_energy", "energy", "guide", "max_violation", "visits"]
    assert default["packed"][0].tolist() == [0, len(rst), 2 * len(rst)] and all(np.array_equal(a, b) for a, b in zip(default["packed"], named["packed"]))
    assert np.array_equal(default["known"], named["known"]) and np.array_equal(default["fixed"], named["fixed"])
    # template: the same held elements, no segment distances, the motif's atoms as targets
    (c,), (samples, info) = run(placement="template", template_weight=2.0, restraints=extra)
    t = structures.motif_template(motif_xyz, segs, weight=2.0)
    assert c["runner"] == "tpl" and c["energy"].shape == (2, 3) and np.array_equal(c["fixed"], default["fixed"]) and np.array_equal(c["known"], default["known"])
    assert c["packed"][0].tolist() == [0, 1, 2] and c["packed"][1].tolist() == [4, 4] and c["packed"][2].tolist() == [46, 46]
    offs, atom, xyz, w = c["tpl_packed"]
    assert offs.tolist() == [0, 24, 48] and np.array_equal(atom[:24], t.atoms) and np.array_equal(atom[24:], t.atoms)
    assert np.array_equal(xyz[24:].view(np.uint64), t.xyz.view(np.uint64)) and (w == 2.0).all()
    assert np.array_equal(info["template_energy"], [7.0, 7.0]) and np.array_equal(info["template_rmsd"], [0.25, 0.25]) and [s.shape for s in samples] == [(24, 6), (30, 6)]
    (c,), _ = run(placement="template")
    assert c["packed"][0].tolist() == [0, 0, 0]
    # both: the segment distances and the template; CA only
    (c,), _ = run(placement="both", template_atoms=("CA",), restraints=extra)
    assert c["runner"] == "tpl" and c["packed"][0].tolist() == [0, len(rst) + 1, 2 * len(rst) + 2]
    assert np.array_equal(c["tpl_packed"][1][:8], structures.motif_template(motif_xyz, segs, atoms=("CA",)).atoms) and c["tpl_packed"][0].tolist() == [0, 8, 16]
    for bad in (dict(placement="mirror"), dict(placement="template", template_weight=0.0), dict(placement="both", template_atoms=("CB",))):
        with pytest.raises(ValueError):
            run(**bad)


def test_guide_inpaint_packs_its_templates_per_batch():
    rng = np.random.default_rng(10)
    known = [random_features(rng, n, 6) for n in (9, 14, 11)]
    fixed = [np.arange(9) % 3 == 1, np.zeros((14, 6), dtype=bool), np.zeros(11, dtype=bool)]
    tpls = [structures.Template([4, 1, 7], rng.standard_normal((3, 3))), None, structures.Template([30], [[1.0, 2.0, 3.0]], 3.0)]
    ds = _dset(OFFSET, T=12)
    run = lambda **kw: sampling.guide_inpaint(_Model(), ds, known, fixed, None, **dict(dict(num_steps=5, batch_size=2, templates=tpls), **kw))   # noqa: E731
    calls, (samples, info) = _recorded(run)
    assert [c["runner"] for c in calls] == ["tpl", "tpl"] and [c["x0"].shape for c in calls] == [(2, 14, 6), (1, 11, 6)]
    assert calls[0]["tpl_packed"][0].tolist() == [0, 3, 3] and calls[0]["tpl_packed"][1].tolist() == [1, 4, 7]
    assert calls[1]["tpl_packed"][0].tolist() == [0, 1] and calls[1]["tpl_packed"][2].tolist() == [[1.0, 2.0, 3.0]] and calls[1]["tpl_packed"][3].tolist() == [3.0]
    assert calls[0]["energy"].shape == (2, 3) and calls[0]["tpl_rmsd"].shape == (2,)
    assert sorted(info) == ["clash_energy", "energy", "guide", "max_violation", "template_energy", "template_rmsd", "visits"]
    assert info["template_energy"].tolist() == [7.0] * 3 and info["template_rmsd"].tolist() == [0.25] * 3 and info["energy"].tolist() == [1.0, 2.0, 1.0]
    plain, _ = _recorded(lambda: run(templates=None))
    assert [c["runner"] for c in plain] == ["plain", "plain"] and np.array_equal(plain[0]["x0"], calls[0]["x0"])   # the same draws either way
    with pytest.raises(ValueError):                        # a template atom beyond its chain, before anything is drawn
        run(templates=structures.Template([27], np.zeros((1, 3))))
    with pytest.raises(ValueError):
        run(templates=tpls[:2])


# ---------------------------------------------------------------------------------- 4. the entries
def test_header_abi_and_binding_hold_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert "#define FDMI_ABI_VERSION 7" in header and lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7
    for name in ("fd_template_energy", "fd_scaffold_guide_step_tpl", "fd_sample_guided_inpaint_tpl"):
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _binding.exported_symbols()
    assert len(_binding._SIGNATURES["fd_scaffold_guide_step_tpl"][1]) == len(_binding._SIGNATURES["fd_scaffold_guide_step"][1]) + 5
    assert len(_binding._SIGNATURES["fd_sample_guided_inpaint_tpl"][1]) == len(_binding._SIGNATURES["fd_sample_guided_inpaint"][1]) + 5
    assert C.sizeof(_binding.FdScaffoldGuideParams) == 9 * 4 + 4 + 16 * 4 + 8 + 24          # no existing struct grew
    assert "OUTSIDE THE DOMAIN" in header and "two largest eigenvalues" in header             # where the energy is not differentiable
    kernels = open(os.path.join(REPO, "foldingdiff_amd", "csrc", "fdmi_kernels.h")).read()
    assert "void launch_template_energy(" in kernels and "template_kernel" in open(os.path.join(REPO, "foldingdiff_amd", "csrc", "template_fit.hip")).read()


P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
f64 = lambda *v: np.array(v, np.float64)                            # noqa: E731
# two chains of 4 and 6 residues, L = 6; chain 0 has two entries, chain 1 three
TPL = dict(offs=i32(0, 2, 5), atom=i32(1, 10, 0, 4, 17), xyz=np.arange(15, dtype=np.float64).reshape(5, 3), w=f64(1, 2, 0.5, 1, 1))
TPL_CASES = [(dict(offs=i32(1, 2, 5)), b"tpl_offsets[0]=1"), (dict(offs=i32(0, 3, 2)), b"tpl_offsets[2]=2 is below"),
             (dict(atom=i32(1, 12, 0, 4, 17)), b"template entry 1 = atom 12 outside chain 0's [0, 12)"),
             (dict(atom=i32(1, 10, 0, 4, 18)), b"template entry 4 = atom 18 outside chain 1's [0, 18)"),
             (dict(atom=i32(-1, 10, 0, 4, 17)), b"template entry 0 = atom -1 outside"),
             (dict(atom=i32(1, 1, 0, 4, 17)), b"template entry 1 = atom 1 after atom 1"), (dict(atom=i32(1, 10, 5, 4, 17)), b"template entry 3 = atom 4 after atom 5"),
             (dict(w=f64(1, 0, 0.5, 1, 1)), b"template entry 1: w=0"), (dict(w=f64(1, 2, -0.5, 1, 1)), b"template entry 2: w=-0.5"),
             (dict(w=f64(1, 2, 0.5, np.inf, 1)), b"template entry 3: w=inf"), (dict(w=f64(np.nan, 2, 0.5, 1, 1)), b"template entry 0: w="),
             (dict(xyz=np.where(np.arange(15).reshape(5, 3) == 7, np.nan, TPL["xyz"])), b"template entry 2: target coordinate 1"),
             (dict(xyz=np.where(np.arange(15).reshape(5, 3) == 12, np.inf, TPL["xyz"])), b"template entry 4: target coordinate 0"),
             (dict(offs=None), b"given together"), (dict(atom=None), b"given together"), (dict(xyz=None), b"given together"), (dict(w=None), b"given together"),
             (dict(offs=None, atom=None, w=None), b"given together")]


def test_fd_template_energy_rejects_bad_arguments_before_touching_a_device(lib):
    """Every rejection of include/fdmi.h returns -1 with its word in fd_last_error() and leaves the outputs alone, on a machine
    without a GPU too.  No valid call is made."""
    B, L = 2, 6
    coords = np.random.default_rng(3).standard_normal((B, 3 * L, 3))
    nan_coords = coords.copy()
    nan_coords[1, 5, 2] = np.nan

    def call(coords=coords, lens=i32(4, 6), B=B, L=L, e="default", r="default", **t):
        a = dict(TPL, **t)
        e, r = (np.full(2, -7.0) if isinstance(v, str) else v for v in (e, r))
        T, g = np.full((2, 12), -7.0), np.full((2, 3 * 6, 3), -7.0)
        return [e, r, T, g], lib.fd_template_energy(0, P(coords), P(lens), B, L, P(a["offs"]), P(a["atom"]), P(a["xyz"]), P(a["w"]), P(e), P(r), P(T), P(g))

    cases = [(dict(coords=None), b"null"), (dict(lens=None), b"null"), (dict(e=None), b"null"), (dict(r=None), b"null"), (dict(B=0), b"B=0"),
             (dict(L=0), b"L=0"), (dict(lens=i32(4, 0)), b"lens[1]=0"), (dict(lens=i32(7, 6)), b"outside [1, 6]"),
             (dict(coords=nan_coords), b"coords is not finite at chain 1, atom 5")] + TPL_CASES
    for kw, word in cases:
        outs, rc = call(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)


def test_the_step_hook_rejects_bad_templates_before_touching_a_device(lib):
    """fd_scaffold_guide_step_tpl: every template rejection, a NULL tpl_rmsd_out, and -- as a sample of what the underlying entry
    rejects, which tests/test_scaffold_guide.py lists in full -- a bad restraint, a bad clash weight and a NaN of x."""
    B, L, F = 2, 6, 6
    x = np.random.default_rng(2).standard_normal((B, L, F)).astype(np.float32)
    nan_x = x.copy()
    nan_x[0, 3, 5] = np.nan
    fixed = np.zeros((B, L, F), np.uint8)
    fixed[0, 1] = 1
    rst = dict(roffs=i32(0, 1, 3), ri=i32(1, 4, 0), rj=i32(10, 16, 17), d0=f64(5, 6, 7), tol=f64(0, 1, 0), rw=f64(1, 0, 2))

    def params(w=1.0):
        p = _binding.FdScaffoldGuideParams()
        p.feat_idx[:] = [int(v) for v in IDX[6]]
        p.max_norm, p.clash_alpha, p.clash_margin, p.w_clash = 1.0, 0.63, 0.15, w
        return p

    def step(x=x, prm=None, rm="default", c=0.1, **kw):
        a = dict(dict(TPL, **rst), **kw)
        prm = params() if prm is None else prm
        out, e, mv, gn, G = np.full((2, L, 16), -7, np.float32), np.full(6, -7.0), np.full(2, -7.0), np.full(2, -7.0), np.full((2, L, 16), -7.0)
        rm = np.full(2, -7.0) if isinstance(rm, str) else rm
        rc = lib.fd_scaffold_guide_step_tpl(0, P(x), P(x), P(x), P(fixed), P(i32(4, 6)), B, L, F, P(np.ones(F, np.uint8)), C.byref(prm), P(a["roffs"]),
                                            P(a["ri"]), P(a["rj"]), P(a["d0"]), P(a["tol"]), P(a["rw"]), P(a["offs"]), P(a["atom"]), P(a["xyz"]), P(a["w"]),
                                            C.c_float(c), C.c_float(0.0), None, C.c_uint64(1), 0, C.c_int64(0), P(out), P(e), P(mv), P(gn), P(G), P(rm))
        return [out, e, mv, gn, G, rm], rc

    cases = TPL_CASES + [(dict(rm=None), b"null"), (dict(ri=i32(12, 4, 0)), b"restraint 0 = atoms (12, 10)"), (dict(prm=params(w=-2.0)), b"w_clash=-2"),
                         (dict(x=nan_x), b"x is not finite at sequence 0, position 3"), (dict(c=np.nan), b"c = ")]
    for kw, word in cases:
        outs, rc = step(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)


def test_the_run_entry_rejects_a_null_model_and_the_script_has_the_flags(lib):
    """A model handle needs a device, so the run's other rejections are in tests/test_template_gpu.py; without one a null handle
    is an argument error and nothing is written."""
    x = np.zeros((1, 4, 6), np.float32)
    out, e, mv, rm = np.full((1, 4, 6), -7, np.float32), np.full(3, -7.0), np.full(1, -7.0), np.full(1, -7.0)
    prm = _binding.FdScaffoldGuideParams()
    rc = lib.fd_sample_guided_inpaint_tpl(None, P(x), P(i32(4)), 1, 4, P(i32(3, 0)), 2, P(np.zeros((5, 2), np.float32)), None, P(x),
                                          P(np.zeros((1, 4, 6), np.uint8)), P(np.zeros(2 * 11, np.float32)), None, C.c_uint64(1), C.c_int64(0),
                                          P(np.zeros(2, np.float32)), C.byref(prm), P(np.zeros(2, np.int32)), None, None, None, None, None,
                                          P(i32(0, 1)), P(i32(1)), P(np.zeros((1, 3))), P(f64(1)), P(out), P(e), P(mv), P(rm))
    assert rc == -1 and lib.fd_last_error() and (out == -7).all() and (e == -7).all() and (mv == -7).all() and (rm == -7).all()
    spec = importlib.util.spec_from_file_location("sample_restrained", os.path.join(REPO, "bin", "sample_restrained.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    motif = ["-m", "x", "-l", "30", "--motif_pdb", "m.pdb", "--motif_residues", "3-6,20-22", "--placed_at", "8,25"]
    args = mod.build_parser().parse_args(motif + ["--placement", "template", "--template_weight", "2.5"])
    assert args.placement == "template" and args.template_weight == 2.5 and args.hold_motif is False
    plain = mod.build_parser().parse_args(motif)
    assert plain.placement is None and plain.template_weight == 1.0
    for argv in (motif + ["--placement", "mirror"], ["-m", "x", "-l", "30", "--contacts", "c.txt", "--placement", "template"],
                 motif + ["--placement", "both", "--template_weight", "0"]):
        with pytest.raises(SystemExit):
            mod.main(argv)
