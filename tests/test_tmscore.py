"""The TM-score's definition on the host: d0, the numpy restatement of the search (tests/tm_reference.py), the Python
argument checks of ``structures.tm_score``, and a static guard on the kernel's registers.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import tm_reference as tr
from conftest import REPO
from foldingdiff_amd import build as fbuild
from foldingdiff_amd import structures


def test_tm_d0():
    assert structures.tm_d0(1) == 0.5 and structures.tm_d0(21) == 0.5
    for Ln in (22, 46, 128, 512):
        assert structures.tm_d0(Ln) == pytest.approx(1.24 * (Ln - 15) ** (1 / 3) - 1.8, rel=1e-15)
        assert structures.tm_d0(Ln) == tr.d0(Ln)
    assert structures.tm_d0(22) == pytest.approx(0.572035, abs=1e-6)
    assert structures.tm_d0(128) == pytest.approx(4.194889, abs=1e-6)


def test_seed_order():
    assert tr.seeds(4) == [(4, 0)]
    assert tr.seeds(9) == [(9, 0)] + [(4, s) for s in range(6)]
    assert tr.seeds(10, stride=4) == [(10, 0), (5, 0), (5, 4), (5, 5), (4, 0), (4, 4), (4, 6)]
    assert len(tr.seeds(128)) == 522


def test_restatement_identity_and_lower_bound():
    rng = np.random.default_rng(1)
    a = tr.ca_chain(rng, 40)
    R0, t0 = tr.rotation(rng), rng.uniform(-30, 30, 3)
    tm, R, t = tr.tm_search(a, a @ R0.T + t0)
    assert tm == pytest.approx(1.0, abs=1e-12)
    assert np.abs(a @ R.T + t - (a @ R0.T + t0)).max() < 1e-9
    for noise in (0.5, 3.0, 8.0):
        b = a @ R0.T + t0 + rng.standard_normal(a.shape) * noise
        tm, R, t = tr.tm_search(a, b, Ln=50)
        Rk, tk = tr.kabsch(a, b)
        assert tm >= tr.tm_of(a, b, Rk, tk, Ln=50)
        assert tm == pytest.approx(tr.tm_of(a, b, R, t, Ln=50), abs=1e-14)


def test_restatement_finds_two_domains():
    """The fixture of the GPU two-domain test: the all-residue fit scores below 0.45, the search at least 0.5."""
    a = tr.ca_chain(np.random.default_rng(0), 120)
    b = tr.two_domain(a, 60)
    Rk, tk = tr.kabsch(a, b)
    assert tr.tm_of(a, b, Rk, tk) < 0.45
    tm, R, t = tr.tm_search(a, b)
    assert tm >= 0.5
    assert np.abs(a[:60] @ R.T + t - b[:60]).max() < 1e-6   # the search superposes the unmoved half


def test_tm_score_checks_shapes_in_python():
    a = np.zeros((5, 3))
    with pytest.raises(ValueError):
        structures.tm_score([a], [np.zeros((4, 3))])
    with pytest.raises(ValueError):
        structures.tm_score([a], [a, a])
    with pytest.raises(ValueError):
        structures.tm_score([np.zeros((5, 2))], [np.zeros((5, 2))])
    with pytest.raises(ValueError):
        structures.tm_score([np.zeros((0, 3))], [np.zeros((0, 3))])
    with pytest.raises(ValueError):
        structures.tm_score([np.zeros((2049, 3))], [np.zeros((2049, 3))])
    with pytest.raises(ValueError):
        structures.tm_score([a], [a], norm_lens=[4])
    with pytest.raises(ValueError):
        structures.tm_score([a], [a], norm_lens=[5, 6])
    with pytest.raises(ValueError):
        structures.tm_score([a], [a], stride=0)


@pytest.fixture(scope="module")
def tm_asm(tmp_path_factory):
    try:
        hipcc = fbuild.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    out = tmp_path_factory.mktemp("isa") / "tm_score.s"
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={fbuild.ARCH}", "-I", os.path.join(REPO, "include"), "-S",
           "--cuda-device-only", "-o", str(out), os.path.join(fbuild.CSRC, "tm_score.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_tm_kernels_hold_no_scratch_and_two_waves_per_simd(tm_asm):
    """No spill in the search (a scratch access per residue would dominate it), and registers for >= 2 waves per
    SIMD: VGPRs + AGPRs, each rounded up to the allocation granule of 8, within 256 of the 512 per lane."""
    meta = {}
    for m in re.finditer(r"\.name:\s+(_Z\S*(tm_score_kernel|tm_reduce_kernel)\S*)\n(.*?)\.wavefront_size", tm_asm, re.S):
        meta[m.group(2)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)", m.group(3))}
    assert sorted(meta) == ["tm_reduce_kernel", "tm_score_kernel"], sorted(meta)
    for name, md in meta.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)
        regs = -(-md["vgpr_count"] // 8) * 8 + -(-md.get("agpr_count", 0) // 8) * 8
        assert 512 // regs >= 2, (name, md)
