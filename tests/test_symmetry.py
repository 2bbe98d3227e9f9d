"""Cyclic oligomers without a device: the symmetry statement of tests/symmetry_reference.py against finite
differences of the coordinates and of the pose, its invariances, the explicit oligomer, the docking descent on the reference
alone, the re-anchoring fit, the builders, the arrays sampling.sample_symmetric prepares (through recording stand-ins), the
assembly PDB writer, the rejections of the new entries (checked on the host before any device call), the header and the
script's flags."""
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
import relax_reference as xr
import symmetry_reference as sr
import template_reference as tr
from conftest import REPO
from foldingdiff_amd import _binding, angles_and_coords, nerf, sampling, structures
from test_guide import IDX, random_features
from test_scaffold_guide import OFFSET, _dset, _Model

PRM = sr.Params()


def chain_and_pose(n, order, seed):
    """A random chain of n residues and a random proper pose that leaves the copies overlapping."""
    rng = np.random.default_rng(seed)
    coords = gr.build_ref(random_features(rng, n, 6), IDX[6])
    coords = coords - coords.mean(axis=0)
    return coords, sr.random_pose(rng, 2.0)


# ---------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("order", [2, 3, 4, 7])
@pytest.mark.parametrize("n", [3, 7, 24, 40])
def test_dcoords_agree_with_finite_differences(n, order):
    """dcoords = Q^T g against central differences of E_clash + E_contact + E_radial over every coordinate, h = 1e-6.  Gate 1e-6 of
    the largest entry, tests/test_scaffold_guide.py's with its derivation (truncation h^2 times a third derivative, rounding
    eps E / h).  Measured over the sixteen cases: at most 3.1e-9 (n = 24, order 7)."""
    coords, pose = chain_and_pose(n, order, 100 * n + order)
    ev = sr.energy(coords, order, pose, PRM)
    assert ev.e[0] > 0 and ev.e[1] < 0 and ev.e[2] > 0
    fd = np.zeros_like(coords)
    h = 1e-6
    for a in range(len(coords)):
        for d in range(3):
            up, down = coords.copy(), coords.copy()
            up[a, d] += h
            down[a, d] -= h
            fd[a, d] = (sr.energy(up, order, pose, PRM).e.sum() - sr.energy(down, order, pose, PRM).e.sum()) / (2 * h)
    scale = np.abs(ev.dcoords).max()
    err = np.abs(ev.dcoords - fd).max() / scale
    print(f"len={n} order={order}: E = {ev.e}, contacts {ev.contacts}, largest entry {scale:.3e}, dcoords against central differences {err:.2e}")
    assert scale > 0 and err <= 1e-6


@pytest.mark.parametrize("n,order", [(3, 2), (7, 3), (24, 4), (40, 7)])
def test_wrench_agrees_with_finite_differences_of_the_pose_and_has_no_z_part(n, order):
    """F = dE/dt and tau = dE/d(a rotation about the origin applied on the left), central differences with h = 1e-6 (gate 1e-6 of
    the largest entry as above; measured at most 2.9e-10), and |F_z| <= 1e-10 |F|, |tau_z| <= 1e-10 |tau| (measured at most 1.4e-15)."""
    coords, pose = chain_and_pose(n, order, 200 * n + order)
    ev = sr.energy(coords, order, pose, PRM)
    Q, t = pose[:9].reshape(3, 3), pose[9:]
    h = 1e-6
    fd = np.zeros(6)
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        moved = [np.concatenate([Q.reshape(9), t + sgn * e]) for sgn in (1, -1)]
        fd[d] = (sr.energy(coords, order, moved[0], PRM).e.sum() - sr.energy(coords, order, moved[1], PRM).e.sum()) / (2 * h)
        turned = [np.concatenate([(sr.rodrigues(sgn * e) @ Q).reshape(9), sr.rodrigues(sgn * e) @ t]) for sgn in (1, -1)]
        fd[3 + d] = (sr.energy(coords, order, turned[0], PRM).e.sum() - sr.energy(coords, order, turned[1], PRM).e.sum()) / (2 * h)
    err = np.abs(ev.wrench - fd).max() / np.abs(ev.wrench).max()
    F, tau = ev.wrench[:3], ev.wrench[3:]
    fz, tz = abs(F[2]) / np.linalg.norm(F), abs(tau[2]) / np.linalg.norm(tau)
    print(f"len={n} order={order}: wrench against central differences {err:.2e}, |F_z|/|F| {fz:.1e}, |tau_z|/|tau| {tz:.1e}")
    assert err <= 1e-6 and fz <= 1e-10 and tz <= 1e-10


@pytest.mark.parametrize("n,order", [(3, 2), (7, 3), (24, 4), (40, 7)])
def test_energy_does_not_change_about_or_along_the_axis(n, order):
    coords, pose = chain_and_pose(n, order, 300 * n + order)
    ev = sr.energy(coords, order, pose, PRM)
    Rz = sr.rodrigues(np.array([0.0, 0.0, 0.83]))
    moved = np.concatenate([(Rz @ pose[:9].reshape(3, 3)).reshape(9), Rz @ pose[9:] + np.array([0.0, 0.0, 17.5])])
    ev2 = sr.energy(coords, order, moved, PRM)
    assert np.allclose(ev2.e, ev.e, rtol=1e-12, atol=0) and ev2.contacts == ev.contacts


@pytest.mark.parametrize("n,order", [(3, 2), (7, 3), (24, 4), (40, 7), (24, 12)])
def test_n_times_the_subunit_energy_is_the_explicit_oligomers(n, order):
    """n (E_clash + E_contact) against the inter-chain sum of structures.cyclic_assembly's chains, and n x contacts / 2 against
    its unordered inter-chain CA pairs below d_on.  Gate 1e-12 relative (measured at most 5.8e-15, at order 12)."""
    coords, pose = chain_and_pose(n, order, 400 * n + order)
    ev = sr.energy(coords, order, pose, PRM)
    chains = structures.cyclic_assembly(coords, pose, order)
    assert chains.shape == (order, 3 * n, 3) and np.allclose(chains, sr.assembly(coords, pose, order), rtol=0, atol=1e-12)
    E, contacts = sr.explicit_interchain(chains, PRM)
    rel = abs(order * (ev.e[0] + ev.e[1]) - E) / abs(E)
    print(f"len={n} order={order}: explicit {E:.6f}, n x subunit {order * (ev.e[0] + ev.e[1]):.6f}, relative {rel:.1e}; contacts {contacts}")
    assert rel <= 1e-12 and order * ev.contacts == 2 * contacts and contacts > 0


def test_order_one_gives_zeros():
    coords, pose = chain_and_pose(7, 1, 5)
    ev = sr.energy(coords, 1, pose, PRM)
    assert not ev.e.any() and ev.contacts == 0 and not ev.wrench.any() and not ev.dcoords.any()


# ---------------------------------------------------------------------------------- 2. the docking descent
# Measured with the default parameters over relax_reference.DEVICE_CHAINS at orders 2 and 3, 100 iterations from
# structures.start_pose: the smallest fall of E over the twelve runs is DOCK_FALL_WORST and the largest count of atoms of one copy
# in a hard clash (fd_backbone_clashes' rule, alpha 0.63) with another is DOCK_CLASHES_WORST; gated at half and at double.
# Measured: E falls by 4.29 (order 3, the 40-residue random chain) to 54.0 (order 3, 128 residues), 80 to 82 of the 100 steps are
# accepted, 46 to 514 contacts, 0 to 21 clashing atoms (21: order 2, 128 residues, whose soft clash energy ends at 4.46).
DOCK_FALL_WORST = 4.2876
DOCK_CLASHES_WORST = 21


@pytest.fixture(scope="module")
def docked():
    runs = []
    for order in (2, 3):
        for ang in xr.device_chains():
            coords = xr.nerf_scan(ang, xr.IDX3)
            pose0 = structures.start_pose([coords], order)[0]
            pose, ev, trace, accepted, h = sr.dock(coords, order, pose0, PRM, 100)
            runs.append(dict(order=order, coords=coords, pose0=pose0, pose=pose, ev=ev, trace=trace, accepted=accepted))
    return runs


def test_the_dock_never_raises_the_energy_and_ends_in_contact(docked):
    falls, clashes = [], []
    for r in docked:
        Q = r["pose"][:9].reshape(3, 3)
        assert (np.diff(r["trace"]) <= 0).all()
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(Q) > 0
        assert r["ev"].contacts > 0
        falls.append(r["trace"][0] - r["trace"][-1])
        clashes.append(sr.hard_clashes_between(sr.assembly(r["coords"], r["pose"], r["order"])))
        print(f"order {r['order']} len {len(r['coords']) // 3}: E {r['trace'][0]:.4f} -> {r['trace'][-1]:.4f}, accepted {r['accepted']}, "
              f"contacts {r['ev'].contacts}, terms {r['ev'].e}, hard clashes {clashes[-1]}")
    print(f"smallest fall {min(falls):.4f}, most hard clashes {max(clashes)}")
    assert min(falls) >= DOCK_FALL_WORST / 2 and max(clashes) <= 2 * DOCK_CLASHES_WORST


def test_a_pose_without_a_wrench_keeps_its_bits():
    pose = sr.random_pose(np.random.default_rng(1), 5.0)
    assert np.array_equal(sr.trial(pose, np.zeros(6), 0.3, PRM), pose)


# ---------------------------------------------------------------------------------- 3. the re-anchoring fit
@pytest.mark.parametrize("n", [7, 24, 40])
def test_the_fit_reanchors_the_pose(n):
    """Unchanged angles: the fit onto Q p + t returns (Q, t) to 1e-12.  After random torsion changes (N(0, 0.1) on every phi and
    psi) the chain placed by the fitted pose lies within the template statement's rmsd of where it was -- that rmsd is the
    root-mean-square distance itself -- and far closer than the chain placed by the OLD pose, which the change at the N-terminus
    has swung away."""
    rng = np.random.default_rng(700 + n)
    ang = random_features(rng, n, 6)
    coords = xr.nerf_scan(ang, IDX[6])
    pose = sr.random_pose(rng, 20.0)
    placed = sr.place(coords, pose)
    same, rmsd0 = sr.fit_pose(coords, placed)
    assert np.abs(same - pose).max() <= 1e-12 * max(1.0, np.abs(pose).max()) and rmsd0 <= 1e-12
    moved = ang.copy()
    moved[:, :2] += rng.normal(0.0, 0.1, size=(n, 2)).astype(np.float32)
    coords2 = xr.nerf_scan(moved, IDX[6])
    pose2, rmsd = sr.fit_pose(coords2, placed)
    Q2 = pose2[:9].reshape(3, 3)
    dev = np.sqrt(((sr.place(coords2, pose2) - placed) ** 2).sum(axis=1).mean())
    stale = np.sqrt(((sr.place(coords2, pose) - placed) ** 2).sum(axis=1).mean())
    print(f"len={n}: rmsd of the fit {rmsd:.3f}, of the re-anchored chain {dev:.3f}, of the stale pose {stale:.3f}")
    assert abs(dev - rmsd) <= 1e-9 * max(1.0, rmsd) and dev <= stale and np.abs(Q2 @ Q2.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(Q2) > 0


# ---------------------------------------------------------------------------------- 4. the builders and the Python surface
def test_start_pose_and_cyclic_assembly():
    rng = np.random.default_rng(4)
    chains = [gr.build_ref(random_features(rng, n, 6), IDX[6]) for n in (9, 20, 5)]
    poses = structures.start_pose(chains, [2, 3, 1])
    assert poses.shape == (3, 12) and poses.dtype == np.float64
    for c, pose, order in zip(chains, poses, (2, 3, 1)):
        ca = c[1::3]
        rg = np.sqrt(((ca - ca.mean(0)) ** 2).sum(1).mean())
        centre = sr.place(c, pose)[1::3].mean(axis=0)
        want = rg / np.sin(np.pi / order) if order >= 2 else 0.0
        assert np.array_equal(pose[:9].reshape(3, 3), np.eye(3)) and np.allclose(centre, [want, 0, 0], atol=1e-9)
    assert np.allclose(sr.place(chains[0], structures.start_pose(chains[:1], 4, radius=12.5)[0])[1::3].mean(0), [12.5, 0, 0], atol=1e-9)
    blind = structures.start_pose(None, [3, 2], lengths=[50, 10])
    assert np.allclose(blind[:, 9:] + nerf.CA_INIT, [[2.2 * 50 ** 0.38 / np.sin(np.pi / 3), 0, 0], [2.2 * 10 ** 0.38, 0, 0]], atol=1e-12)
    asm = structures.cyclic_assembly(chains[1], poses[1], 3)
    assert asm.shape == (3, 60, 3) and np.allclose(asm[0], sr.place(chains[1], poses[1]))
    assert np.allclose(asm[1] @ sr.rot_z(1, 3).T, asm[2]) and np.allclose(asm[2] @ sr.rot_z(1, 3).T, asm[0], atol=1e-9)
    for bad in (0, 13):
        with pytest.raises(ValueError):
            structures.start_pose(chains[:1], bad)
        with pytest.raises(ValueError):
            structures.cyclic_assembly(chains[0], poses[0], bad)
    with pytest.raises(ValueError):
        structures.start_pose(None, 3)
    prm = structures.symmetry_params()
    assert (prm.w_clash, prm.w_contact, prm.d_on, prm.d_off, prm.w_radial, prm.r_max) == (1.0, 0.1, 8.0, 12.0, 0.01, 0.0)
    assert (prm.lever, prm.max_shift, prm.step0, prm.grow, prm.shrink, prm.pose_iters) == (10.0, 1.0, 0.01, 1.2, 0.5, 1)
    assert (prm.clash_alpha, prm.clash_margin) == (PRM.alpha, PRM.margin) and tuple(PRM[2:]) == (1.0, 0.1, 8.0, 12.0, 0.01, 0.0, 10.0, 1.0, 0.01, 1.2, 0.5, 1)


def _recorded(fn):
    """The arguments of every runner call ``fn`` makes, with stand-ins that copy x0 into out; the symmetric runner reports the
    start pose shifted by 1 along z."""
    calls = []
    sigs = {name: inspect.signature(getattr(sampling, f"_run_fd_sample_guided_inpaint{suffix}"))
            for name, suffix in (("plain", ""), ("tpl", "_tpl"), ("sym", "_sym"))}

    def stand_in(name):
        def run(*args, **kwargs):
            a = dict(sigs[name].bind(*args, **kwargs).arguments)
            calls.append(dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}, runner=name))
            a["out"][...] = a["x0"]
            a["energy"][:, 0], a["energy"][:, 1], a["worst"][:] = 1.0 + np.arange(len(a["worst"])), 0.5, 2.0
            if name != "plain":
                a["energy"][:, 2], a["tpl_rmsd"][:] = 7.0, 0.25
            if name == "sym":
                a["sym_energy"][:], a["sym_contacts"][:], a["sym_pose"][:] = (3.0, -2.0, 1.0), 11, a["pose0"] + np.eye(12)[11]
        return run
    with mock.patch.object(sampling, "_run_fd_sample_guided_inpaint", stand_in("plain")), \
            mock.patch.object(sampling, "_run_fd_sample_guided_inpaint_tpl", stand_in("tpl")), \
            mock.patch.object(sampling, "_run_fd_sample_guided_inpaint_sym", stand_in("sym")):
        torch.manual_seed(7)
        returned = fn()
    return calls, returned


def test_guide_inpaint_takes_a_symmetry_and_is_unchanged_without_one():
    rng = np.random.default_rng(10)
    known = [random_features(rng, n, 6) for n in (9, 14, 11)]
    fixed = [np.arange(9) % 3 == 1, np.zeros((14, 6), dtype=bool), np.zeros(11, dtype=bool)]
    ds = _dset(OFFSET, T=12)
    prm = structures.symmetry_params(pose_iters=2)
    run = lambda **kw: sampling.guide_inpaint(_Model(), ds, known, fixed, None, num_steps=5, batch_size=2, **kw)   # noqa: E731
    calls, (samples, info) = _recorded(lambda: run(symmetry={"order": [3, 1, 4], "params": prm}))
    assert [c["runner"] for c in calls] == ["sym", "sym"] and [c["x0"].shape for c in calls] == [(2, 14, 6), (1, 11, 6)]
    assert calls[0]["order"].tolist() == [3, 1] and calls[1]["order"].tolist() == [4] and calls[0]["order"].dtype == np.int32
    assert calls[0]["tpl_packed"] == (None,) * 4 and calls[0]["sym_params"] is prm and calls[0]["energy"].shape == (2, 3)
    want = structures.start_pose(None, [3, 1, 4], lengths=[9, 14, 11])
    assert np.array_equal(calls[0]["pose0"], want[:2]) and np.array_equal(calls[1]["pose0"], want[2:]) and calls[0]["pose0"].flags.c_contiguous
    assert sorted(info) == ["clash_energy", "energy", "guide", "max_violation", "symmetry_contacts", "symmetry_energy", "symmetry_pose", "visits"]
    assert info["symmetry_energy"].shape == (3, 3) and info["symmetry_contacts"].tolist() == [11] * 3
    assert np.array_equal(info["symmetry_pose"], want + np.eye(12)[11])
    plain, (_, plain_info) = _recorded(lambda: run())
    assert [c["runner"] for c in plain] == ["plain", "plain"] and np.array_equal(plain[0]["x0"], calls[0]["x0"])   # the same draws either way
    assert sorted(plain_info) == ["clash_energy", "energy", "guide", "max_violation", "visits"] and plain[0]["energy"].shape == (2, 2)
    both, (_, both_info) = _recorded(lambda: run(symmetry={"order": 2, "pose": want}, templates=structures.Template([4, 1], np.zeros((2, 3)))))
    assert [c["runner"] for c in both] == ["sym", "sym"] and both[0]["tpl_packed"][0].tolist() == [0, 2, 4] and "template_rmsd" in both_info
    for bad in ({"order": 13}, {"order": [2, 2]}, {"pose": want}, {"order": 2, "radius": 3.0}, {"order": 2, "pose": want[:2]},
                {"order": 2, "pose": np.where(np.arange(36).reshape(3, 12) == 5, np.nan, want)}):
        with pytest.raises(ValueError):
            run(symmetry=bad)


def test_sample_symmetric_holds_nothing_and_docks_from_the_runs_pose():
    ds = _dset(OFFSET, T=12)
    docks, builds = [], []

    def dock_stand_in(coords, order, pose=None, n_iter=100, params=None, **kw):
        docks.append(dict(coords=coords, order=order, pose=pose, n_iter=n_iter, params=params, device=kw.get("device")))
        B = len(coords)
        return structures.DockResult(pose + np.eye(12)[9], np.full((B, 3), 5.0), np.full(B, 4, dtype=np.int32), np.zeros(B, dtype=np.int64),
                                     np.full(B, 0.01), None)

    def build_stand_in(angles, names, center_coords=True, device=0, method="serial"):
        builds.append(dict(center=center_coords, method=method, device=device))
        return [np.zeros((3 * len(a), 3)) for a in angles]

    prm = structures.symmetry_params()
    with mock.patch.object(structures, "dock_cyclic", dock_stand_in), mock.patch.object(nerf, "build_backbones", build_stand_in):
        calls, res = _recorded(lambda: sampling.sample_symmetric(_Model(), ds, [12, 20], order=3, num_steps=4, symmetry_params=prm, dock_iters=30))
    (c,) = calls
    assert c["runner"] == "sym" and not c["fixed"].any() and c["packed"][0].tolist() == [0, 0, 0] and c["order"].tolist() == [3, 3]
    assert c["params"].w_clash == 1.0 and c["sym_params"] is prm and len(c["visits"]) == 4
    assert builds == [dict(center=False, method="scan", device=0)]                    # (the stand-in model is on no GPU)
    (d,) = docks
    assert d["device"] == 0 and d["n_iter"] == 30 and d["params"] is prm and np.array_equal(d["pose"], res.info["symmetry_pose"]) and [len(x) for x in d["coords"]] == [36, 60]
    assert np.array_equal(res.pose, res.info["symmetry_pose"] + np.eye(12)[9]) and res.contacts.tolist() == [4, 4] and res.order.tolist() == [3, 3]
    assert [a.shape for a in res.angles] == [(12, 6), (20, 6)] and res.energy.shape == (2, 3)
    with mock.patch.object(structures, "dock_cyclic", dock_stand_in), mock.patch.object(nerf, "build_backbones", build_stand_in):
        _recorded(lambda: sampling.sample_symmetric(_Model(), ds, [12], order=2, num_steps=4, dock_iters=1, device=3))
    assert builds[-1]["device"] == 3 and docks[-1]["device"] == 3


def test_write_assembly_pdb_writes_one_chain_per_copy(tmp_path):
    rng = np.random.default_rng(3)
    coords = gr.build_ref(random_features(rng, 11, 6), IDX[6])
    chains = structures.cyclic_assembly(coords, structures.start_pose([coords], 4)[0], 4)
    fname = angles_and_coords.write_assembly_pdb(chains, str(tmp_path / "asm.pdb"))
    lines = open(fname).read().splitlines()
    atoms = [l for l in lines if l.startswith("ATOM")]
    ters = [l for l in lines if l.startswith("TER")]
    assert len(atoms) == 4 * 33 and [l[21] for l in ters] == list("ABCD") and lines[-1] == "END"
    assert [l[21] for l in atoms] == [ch for ch in "ABCD" for _ in range(33)] and [int(l[6:11]) for l in atoms[:34]] == list(range(1, 34)) + [35]
    assert all(len(l) == 80 for l in atoms) and [int(l[22:26]) for l in atoms[33:39]] == [1, 1, 1, 2, 2, 2]
    single = angles_and_coords.write_coords_to_pdb(chains[0], str(tmp_path / "one.pdb"))
    assert open(single).read().splitlines()[:33] == atoms[:33]                     # the existing writer's ATOM line layout
    for k, ch in enumerate("ABCD"):
        assert np.abs(angles_and_coords.read_pdb_backbone(fname, chain=ch) - chains[k]).max() <= 5e-4 + 1e-12
    assert angles_and_coords.read_pdb_backbone(fname).shape == (132, 3)
    with pytest.raises(AssertionError):
        angles_and_coords.write_assembly_pdb([coords] * 27, str(tmp_path / "many.pdb"))


# ---------------------------------------------------------------------------------- 5. the entries
def test_header_abi_and_binding_hold_the_new_entries(lib):
    header = open(os.path.join(REPO, "include", "fdmi.h")).read()
    assert "#define FDMI_ABI_VERSION 7" in header and lib.fd_abi_version() == 7 and _binding.ABI_VERSION == 7
    for name in ("fd_symmetry_energy", "fd_symmetry_dock", "fd_scaffold_guide_step_sym", "fd_sample_guided_inpaint_sym"):
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _binding.exported_symbols()
    assert len(_binding._SIGNATURES["fd_scaffold_guide_step_sym"][1]) == len(_binding._SIGNATURES["fd_scaffold_guide_step_tpl"][1]) + 9
    assert len(_binding._SIGNATURES["fd_sample_guided_inpaint_sym"][1]) == len(_binding._SIGNATURES["fd_sample_guided_inpaint_tpl"][1]) + 6
    assert C.sizeof(_binding.FdSymmetryParams) == 13 * 8 + 8 and "typedef struct fd_symmetry_params" in header
    assert C.sizeof(_binding.FdScaffoldGuideParams) == 9 * 4 + 4 + 16 * 4 + 8 + 24          # no existing struct grew
    for phrase in ("a == b included", "F == tau == 0 keeps the pose's bits", "Q = R^T, t = -R^T t_fit", "block coordinate descent"):
        assert phrase in header, phrase
    kernels = open(os.path.join(REPO, "foldingdiff_amd", "csrc", "fdmi_kernels.h")).read()
    source = open(os.path.join(REPO, "foldingdiff_amd", "csrc", "symmetry.hip")).read()
    assert "void launch_symmetry_pair(" in kernels and "void launch_symmetry_pose(" in kernels and "void launch_symmetry_place(" in kernels
    assert all(k in source for k in ("symmetry_pair_kernel", "symmetry_pose_kernel", "symmetry_place_kernel")) and "atomic" not in source.replace("atomics", "")
    from foldingdiff_amd import build
    assert "symmetry.hip" in build.SOURCES


P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
f64 = lambda *v: np.array(v, np.float64)                            # noqa: E731
POSES = np.tile(np.concatenate([np.eye(3).reshape(9), [4.0, 0.0, 0.0]]), (2, 1))


def sym_params(**kw):
    p = structures.symmetry_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def nan_at(a, *index):
    out = np.array(a, dtype=np.float64)
    out[index] = np.nan
    return out


# what check_symmetry rejects, shared by the four entries: (the changed arguments, the word in fd_last_error())
SYM_CASES = [(dict(prm=sym_params(**{k: v})), f"{k}=".encode()) for k in ("clash_alpha", "clash_margin", "w_clash", "w_contact", "w_radial", "r_max")
             for v in (-1.0, np.nan, np.inf)]
SYM_CASES += [(dict(prm=sym_params(d_on=-1.0)), b"d_on=-1"), (dict(prm=sym_params(d_on=12.0)), b"d_on=12"), (dict(prm=sym_params(d_off=np.inf)), b"d_off=inf"),
              (dict(prm=sym_params(d_on=np.nan)), b"d_on=nan"), (dict(prm=sym_params(lever=0.0)), b"lever=0"), (dict(prm=sym_params(max_shift=-1.0)), b"max_shift=-1"),
              (dict(prm=sym_params(step0=0.0)), b"step0=0"), (dict(prm=sym_params(step0=np.inf)), b"step0=inf"), (dict(prm=sym_params(grow=0.99)), b"grow=0.99"),
              (dict(prm=sym_params(shrink=1.0)), b"shrink=1"), (dict(prm=sym_params(shrink=0.0)), b"shrink=0"), (dict(prm=sym_params(pose_iters=-1)), b"pose_iters=-1"),
              (dict(order=i32(0, 3)), b"order[0]=0"), (dict(order=i32(2, 13)), b"order[1]=13"), (dict(pose=nan_at(POSES, 1, 4)), b"pose[1][4]"),
              (dict(pose=np.where(np.arange(24).reshape(2, 12) == 9, np.inf, POSES)), b"pose[0][9]")]


def test_the_model_free_entries_reject_bad_arguments_before_touching_a_device(lib):
    """Every rejection of include/fdmi.h returns -1 with its word in fd_last_error() and leaves the outputs alone, on a machine
    without a GPU too.  No valid call is made."""
    B, L = 2, 6
    coords = np.random.default_rng(3).standard_normal((B, 3 * L, 3))

    def energy(coords=coords, lens=i32(4, 6), B=B, L=L, order=i32(2, 3), pose=POSES, prm="default", e="default", c="default", **_):
        prm = sym_params() if isinstance(prm, str) else prm
        e, c = (np.full(6, -7.0) if isinstance(e, str) else e), (np.full(2, -7, np.int32) if isinstance(c, str) else c)
        w, g = np.full((2, 6), -7.0), np.full((2, 3 * 6, 3), -7.0)
        return [e, c, w, g], lib.fd_symmetry_energy(0, P(coords), P(lens), B, L, P(order), P(pose), None if prm is None else C.byref(prm), P(e), P(c), P(w), P(g))

    def dock(coords=coords, lens=i32(4, 6), B=B, L=L, order=i32(2, 3), pose=POSES, prm="default", e="default", c="default", n_iter=3, step="default",
             po="default", acc="default"):
        prm = sym_params() if isinstance(prm, str) else prm
        e, c = (np.full(6, -7.0) if isinstance(e, str) else e), (np.full(2, -7, np.int32) if isinstance(c, str) else c)
        po, acc = (np.full((2, 12), -7.0) if isinstance(po, str) else po), (np.full(2, -7, np.int32) if isinstance(acc, str) else acc)
        step = np.full(2, 0.01) if isinstance(step, str) else step
        before = None if step is None else step.copy()
        tr_ = np.full((n_iter + 1 if n_iter >= 0 else 1, 2), -7.0)
        rc = lib.fd_symmetry_dock(0, P(coords), P(lens), B, L, P(order), P(pose), None if prm is None else C.byref(prm), n_iter, P(step), P(po), P(e), P(c),
                                  P(tr_), P(acc))
        assert before is None or np.array_equal(step, before, equal_nan=True)
        return [e, c, po, acc, tr_], rc

    shared = [(dict(coords=None), b"null"), (dict(lens=None), b"null"), (dict(order=None), b"null"), (dict(pose=None), b"null"), (dict(prm=None), b"null"),
              (dict(e=None), b"null"), (dict(c=None), b"null"), (dict(B=0), b"B=0"), (dict(L=0), b"L=0"), (dict(lens=i32(4, 0)), b"lens[1]=0"),
              (dict(lens=i32(7, 6)), b"outside [1, 6]"), (dict(coords=nan_at(coords, 1, 5, 2)), b"coords is not finite at chain 1, atom 5")] + SYM_CASES
    own = [(dict(n_iter=-1), b"n_iter=-1"), (dict(step=f64(0.01, 0.0)), b"step_io[1]=0"), (dict(step=f64(np.nan, 0.01)), b"step_io[0]="),
           (dict(po=None), b"null"), (dict(acc=None), b"null")]
    for entry, cases in ((energy, shared), (dock, shared + own)):
        for kw, word in cases:
            outs, rc = entry(**kw)
            msg = lib.fd_last_error()
            assert rc == -1 and msg and word in msg, (entry.__name__, word, rc, msg)
            assert all((o == -7).all() for o in outs if o is not None), (entry.__name__, word, msg)


def test_the_step_hook_rejects_bad_symmetry_arguments_before_touching_a_device(lib):
    """fd_scaffold_guide_step_sym: every symmetry rejection, a missing symmetry array, and -- as a sample of what the underlying
    entries reject, which tests/test_scaffold_guide.py and tests/test_template.py list in full -- a bad restraint, a bad template
    and a NaN of x."""
    B, L, F = 2, 6, 6
    x = np.random.default_rng(2).standard_normal((B, L, F)).astype(np.float32)
    fixed = np.zeros((B, L, F), np.uint8)
    placed = np.random.default_rng(4).standard_normal((B, 3 * L, 3))
    gp = _binding.FdScaffoldGuideParams()
    gp.feat_idx[:] = [int(v) for v in IDX[6]]
    gp.max_norm, gp.clash_alpha, gp.clash_margin, gp.w_clash = 1.0, 0.63, 0.15, 1.0

    def step(x=x, order=i32(2, 3), pose=POSES, placed=placed, prm="default", h="default", se="default", sc="default", sp="default", spl="default",
             roffs=i32(0, 0, 0), tpl=(None,) * 4, c=0.1):
        prm = sym_params() if isinstance(prm, str) else prm
        h = np.full(2, 0.01) if isinstance(h, str) else h
        out, e, mv, gn, G, rm = np.full((2, L, 16), -7, np.float32), np.full(6, -7.0), np.full(2, -7.0), np.full(2, -7.0), np.full((2, L, 16), -7.0), np.full(2, -7.0)
        se, sc = (np.full(6, -7.0) if isinstance(se, str) else se), (np.full(2, -7, np.int32) if isinstance(sc, str) else sc)
        sp, spl = (np.full((2, 12), -7.0) if isinstance(sp, str) else sp), (np.full((2, 3 * L, 3), -7.0) if isinstance(spl, str) else spl)
        before = None if h is None else h.copy()
        rc = lib.fd_scaffold_guide_step_sym(0, P(x), P(x), P(x), P(fixed), P(i32(4, 6)), B, L, F, P(np.ones(F, np.uint8)), C.byref(gp), P(roffs), None, None,
                                            None, None, None, *(P(t) for t in tpl), P(order), P(pose), P(placed), None if prm is None else C.byref(prm), P(h),
                                            C.c_float(c), C.c_float(0.0), None, C.c_uint64(1), 0, C.c_int64(0), P(out), P(e), P(mv), P(gn), P(G), P(rm), P(se),
                                            P(sc), P(sp), P(spl))
        assert before is None or np.array_equal(h, before, equal_nan=True)
        return [out, e, mv, gn, G, rm, se, sc, sp, spl], rc

    cases = SYM_CASES + [(dict(pose=None), b"symmetry arrays"), (dict(prm=None), b"symmetry arrays"), (dict(se=None), b"symmetry arrays"),
                         (dict(sc=None), b"symmetry arrays"), (dict(sp=None), b"symmetry arrays"), (dict(spl=None), b"symmetry arrays"),
                         (dict(h=f64(0.01, -1.0)), b"sym_step_io[1]=-1"), (dict(placed=nan_at(placed, 0, 11, 1)), b"sym_placed_in is not finite at chain 0, atom 11"),
                         (dict(roffs=i32(0, 2, 1)), b"rst_offsets[2]=1 is below"), (dict(tpl=(i32(0, 1, 1), None, None, None)), b"given together"),
                         (dict(x=nan_at(x, 0, 3, 5).astype(np.float32)), b"x is not finite at sequence 0, position 3"), (dict(c=np.nan), b"c = ")]
    for kw, word in cases:
        outs, rc = step(**kw)
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)


def test_the_run_entry_rejects_a_null_model_and_the_script_has_the_flags(lib):
    """A model handle needs a device, so the run's other rejections are in tests/test_symmetry_gpu.py; without one a null handle is
    an argument error and nothing is written."""
    x = np.zeros((1, 4, 6), np.float32)
    out, e, mv, rm = np.full((1, 4, 6), -7, np.float32), np.full(3, -7.0), np.full(1, -7.0), np.full(1, -7.0)
    se, sc, sp = np.full(3, -7.0), np.full(1, -7, np.int32), np.full(12, -7.0)
    gp, prm = _binding.FdScaffoldGuideParams(), structures.symmetry_params()
    rc = lib.fd_sample_guided_inpaint_sym(None, P(x), P(i32(4)), 1, 4, P(i32(3, 0)), 2, P(np.zeros((5, 2), np.float32)), None, P(x),
                                          P(np.zeros((1, 4, 6), np.uint8)), P(np.zeros(2 * 11, np.float32)), None, C.c_uint64(1), C.c_int64(0),
                                          P(np.zeros(2, np.float32)), C.byref(gp), P(np.zeros(2, np.int32)), None, None, None, None, None,
                                          None, None, None, None, P(i32(3)), P(POSES[:1].copy()), C.byref(prm), P(out), P(e), P(mv), P(rm), P(se), P(sc), P(sp))
    assert rc == -1 and lib.fd_last_error() and all((o == -7).all() for o in (out, e, mv, rm, se, sc, sp))
    spec = importlib.util.spec_from_file_location("sample_symmetric", os.path.join(REPO, "bin", "sample_symmetric.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args(["-m", "x", "-l", "60", "--order", "4", "--num_steps", "20", "--eta", "0.5", "--dock_iters", "40"])
    assert (args.length, args.order, args.num_steps, args.eta, args.dock_iters, args.pose_iters) == (60, 4, 20, 0.5, 40, 1)
    assert mod.build_parser().parse_args(["-m", "x", "-l", "60"]).order == 3
    for argv in (["-m", "x", "-l", "60", "--order", "1"], ["-m", "x", "-l", "60", "--order", "13"], ["-m", "x", "-l", "0"], ["-m", "x", "-l", "60", "--dock_iters", "-1"]):
        with pytest.raises(SystemExit):
            mod.main(argv)
