"""The C-ABI library loads (no GPU needed) and exports exactly what include/fdmi.h declares."""
import os
import re

from conftest import REPO
from foldingdiff_amd import _binding


def _declared():
    src = open(os.path.join(REPO, "include", "fdmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fd_[a-z_0-9]+)\s*\(", src)))


def test_header_and_binding_agree(lib):
    declared = _declared()
    assert declared, "no declarations parsed"
    assert sorted(_binding.exported_symbols()) == declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in fdmi.h but not exported by libfdmi.so"


def test_abi_version_and_error_string(lib):
    assert lib.fd_abi_version() == _binding.ABI_VERSION
    assert lib.fd_device_count() >= 0
    # argument errors are reported through codes + fd_last_error, never by crashing
    rc = lib.fd_create(None, 0, None)
    assert rc == -1 and b"null" in lib.fd_last_error()
    rc = lib.fd_profile_every(None, 1)
    assert rc == -1


def test_debug_read_rejects_a_null_model(lib):
    """fd_debug_read without a model: -1, "null" in fd_last_error(), the output left alone.  This is all that can be asked without
    a device (no model can be created), and it does not reach the "scales" branch: its own bad-argument cases -- an unfinalized
    model, a short buffer, a debug_layer that names no layer, a model finalized in FD_PREC_F32 -- need a model and are in
    tests/test_gpu_parity.py::test_debug_read_scales_arguments."""
    import ctypes as C

    import numpy as np

    out = np.full(21, -7, np.float32)
    rc = lib.fd_debug_read(None, b"scales", out.ctypes.data_as(C.c_void_p), out.size)
    assert rc == -1 and b"null" in lib.fd_last_error(), (rc, lib.fd_last_error())
    assert (out == -7).all()


def test_model_free_entries_reject_bad_arguments_before_touching_a_device(lib):
    """The ten entries that take a device_id check every argument before their first HIP call: each bad call returns
    -1 with its word in fd_last_error() and leaves the outputs alone, on a machine without a GPU too.  No valid call
    is made.  Two chains of 4 and 6 residues; the hooks get K = 8."""
    import ctypes as C

    import numpy as np

    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)                              # noqa: E731
    ca = np.random.default_rng(5).standard_normal((10, 3))
    offs, lens, pa, pb = i32(0, 4), i32(4, 6), i32(0, 1), i32(1, 0)
    bad_nan = ca.copy()
    bad_nan[7, 1] = np.nan
    checked = 0

    def expect(word, outs, rc):
        nonlocal checked
        msg = lib.fd_last_error()
        assert rc == -1 and msg and word in msg, (word, rc, msg)
        assert all((o == -7).all() for o in outs if o is not None), (word, msg)
        checked += 1

    # ---- the CA-trace entries
    def tm_score(a=ca, b=ca, offs=offs, lens=lens, norm=None, n=2, stride=1, out="default"):
        tm, T = (np.full(2, -7.0) if isinstance(out, str) else out), np.full((2, 12), -7.0)
        return [tm, T], lib.fd_tm_score(0, P(a), P(b), P(offs), P(lens), P(norm), n, stride, P(tm), P(T))

    for kw, word in [(dict(a=None), b"null"), (dict(b=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"),
                     (dict(out=None), b"null"), (dict(n=0), b"n_pairs"), (dict(stride=0), b"stride"),
                     (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(2049, 6)), b"outside [1, 2048]"),
                     (dict(offs=i32(0, 5)), b"offsets"), (dict(norm=i32(4, 5)), b"norm_lens"),
                     (dict(a=bad_nan), b"finite"), (dict(b=bad_nan), b"finite")]:
        expect(word, *tm_score(**kw))

    def annotate(ca=ca, offs=offs, lens=lens, n=2, sse="default"):
        sse, counts = (np.full(10, -7, np.int8) if isinstance(sse, str) else sse), np.full((2, 2), -7, np.int32)
        return [sse, counts], lib.fd_annotate_sse(0, P(ca), P(offs), P(lens), n, P(sse), P(counts))

    for kw, word in [(dict(ca=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(sse=None), b"null"),
                     (dict(n=0), b"n_chains"), (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(2049, 6)), b"outside [1, 2048]"),
                     (dict(offs=i32(0, 5)), b"offsets"), (dict(ca=bad_nan), b"finite")]:
        expect(word, *annotate(**kw))

    def align(ca=ca, offs=offs, lens=lens, nc=2, pa=pa, pb=pb, norm=None, n=2, max_iter=3, out="default",
              moff=np.array([0, 4], np.int64), use_map=True):
        tm = np.full(2, -7.0) if isinstance(out, str) else out
        T, n_ali, amap = np.full((2, 12), -7.0), np.full(2, -7, np.int32), np.full(10, -7, np.int32)
        return [tm, T, n_ali, amap], lib.fd_tm_align(0, P(ca), P(offs), P(lens), nc, P(pa), P(pb), P(norm), n, max_iter, P(tm),
                                                     P(T), P(n_ali), P(moff), P(amap) if use_map else None)

    for kw, word in [(dict(ca=None), b"null"), (dict(offs=None), b"null"), (dict(lens=None), b"null"), (dict(pa=None), b"null"),
                     (dict(pb=None), b"null"), (dict(out=None), b"null"), (dict(use_map=False), b"null"), (dict(moff=None), b"null"),
                     (dict(n=0), b"n_pairs"), (dict(nc=0), b"n_chains"), (dict(max_iter=0), b"max_iter"),
                     (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(513, 4)), b"outside [1, 512]"),
                     (dict(offs=i32(0, 5)), b"offsets"), (dict(pa=i32(0, 2)), b"chain index"),
                     (dict(norm=i32(4, 3)), b"norm_lens"), (dict(moff=np.array([0, 5], np.int64)), b"map_offsets"),
                     (dict(ca=bad_nan), b"finite")]:
        expect(word, *align(**kw))

    # ---- the packed entries without a length cap: the same 10 x 3 array as ten fp64 atoms, and as float32 coordinates
    def rmsd(a=ca, b=ca, offs=offs, lens=lens, n=2, out="default"):
        out = np.full(2, -7.0) if isinstance(out, str) else out
        return [out], lib.fd_superpose_rmsd(0, P(a), P(b), P(offs), P(lens), n, P(out))

    for kw, word in [(dict(a=None), b"bad argument"), (dict(b=None), b"bad argument"), (dict(offs=None), b"bad argument"),
                     (dict(lens=None), b"bad argument"), (dict(out=None), b"bad argument"), (dict(n=0), b"bad argument"),
                     (dict(lens=i32(4, 0)), b"lens"), (dict(offs=i32(0, 5)), b"offsets")]:
        expect(word, *rmsd(**kw))

    xyz = np.zeros((90, 3), np.float32)   # 10 residues x (N, CA, C)

    def coords(xyz=xyz, offs=offs, lens=lens, n=2, out="default"):
        out = np.full((10, 9), -7, np.float32) if isinstance(out, str) else out
        return [out], lib.fd_internal_coords(0, P(xyz), P(offs), P(lens), n, P(out))

    for kw, word in [(dict(xyz=None), b"bad argument"), (dict(offs=None), b"bad argument"), (dict(lens=None), b"bad argument"),
                     (dict(out=None), b"bad argument"), (dict(n=0), b"bad argument"), (dict(lens=i32(4, 0)), b"lens"),
                     (dict(offs=i32(0, 5)), b"offsets")]:
        expect(word, *coords(**kw))

    # ---- fd_nerf: B = 2, L = 6, F = 6
    feats, idx = np.zeros((2, 6, 6), np.float32), i32(0, 1, 2, 3, 4, 5, -1, -1, -1)

    def nerf(feats=feats, lens=lens, B=2, idx=idx, out="default"):
        out = np.full((2, 18, 3), -7.0) if isinstance(out, str) else out
        return [out], lib.fd_nerf(0, P(feats), P(lens), B, 6, 6, P(idx), 1, P(out))

    for kw, word in [(dict(feats=None), b"bad argument"), (dict(lens=None), b"bad argument"), (dict(idx=None), b"bad argument"),
                     (dict(out=None), b"bad argument"), (dict(B=0), b"bad argument"),
                     (dict(idx=i32(6, 1, 2, 3, 4, 5, -1, -1, -1)), b"feat_idx"),
                     (dict(lens=i32(4, 0)), b"lens"), (dict(lens=i32(4, 7)), b"outside [1, 6]")]:
        expect(word, *nerf(**kw))

    # ---- the hooks: K = 8 is below every kernel's k-tile
    v = np.zeros(16, np.float32)
    for src, n, dst in [(None, 16, np.full(16, -7, np.float32)), (v, 16, None), (v, 0, np.full(16, -7, np.float32))]:
        expect(b"bad argument", [dst], lib.fd_test_wrap(0, 0, P(src), n, P(dst)))

    A, W, bias, R = (np.zeros(s, np.float32) for s in ((4, 32), (32, 32), (32,), (4, 32)))

    def gemm(A=A, W=W, bias=bias, R=R, out="default", epi=0, M=4, K=32):
        out = np.full((4, 32), -7, np.float32) if isinstance(out, str) else out
        return [out], lib.fd_test_gemm(0, 0, epi, P(A), P(W), P(bias), P(R), P(out), M, 32, K)

    def gemm_ln(A=A, W=W, bias=bias, R=R, g=bias, b=bias, out="default", M=4, K=32, prec=0):
        out = np.full((4, 32), -7, np.float32) if isinstance(out, str) else out
        return [out], lib.fd_test_gemm_ln(0, prec, 1, P(A), P(W), P(bias), P(R), P(g), P(b), C.c_float(1e-12), P(out), M, 32, K)

    for kw, word in [(dict(A=None), b"bad argument"), (dict(W=None), b"bad argument"), (dict(bias=None), b"bad argument"),
                     (dict(out=None), b"bad argument"), (dict(M=0), b"bad argument"), (dict(K=8), b"bad argument"),
                     (dict(epi=2, R=None), b"bad epilogue"), (dict(epi=3), b"bad epilogue")]:
        expect(word, *gemm(**kw))
    for kw, word in [(dict(A=None), b"bad argument"), (dict(W=None), b"bad argument"), (dict(bias=None), b"bad argument"),
                     (dict(R=None), b"bad argument"), (dict(g=None), b"bad argument"), (dict(b=None), b"bad argument"),
                     (dict(out=None), b"bad argument"), (dict(M=0), b"bad argument"), (dict(K=8), b"bad argument"),
                     (dict(prec=7), b"precision")]:
        expect(word, *gemm_ln(**kw))
    ms = C.c_double(-7.0)
    for args in [(0, 4, 32, 8, 1), (0, 0, 32, 32, 1), (0, 4, 32, 32, 0)]:
        expect(b"bad argument", [], lib.fd_test_gemm_time(0, *args, C.byref(ms)))
        assert ms.value == -7.0
    expect(b"bad argument", [], lib.fd_test_gemm_time(0, 0, 4, 32, 32, 1, None))
    assert checked == 13 + 9 + 18 + 8 + 7 + 8 + 3 + 8 + 10 + 4
