"""The real weight packer (csrc/weight_pack.h) from Python, for tests/test_weight_pack.py, tests/test_host.py and
tests/golden/make_golden_weight_images.py: the shim's build, its ctypes wrappers, matrices whose packed halves say where they
came from, and the fixed inputs of the golden hashes.  CPU only."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

from foldingdiff_amd import build as fbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "weight_pack_shim.cpp")
GOLDEN = os.path.join(HERE, "golden", "weight_images.json")
SHAPES = ((64, 128), (192, 384), (384, 768))   # (d_model, d_ff): nkt = 2 (an interior and a last group), 6 (odd nkt / 2), 12 (released)


def find_clangxx() -> str:
    """The clang++ that ships with ROCm, beside the hipcc that the build uses (the system g++ may lack _Float16).
    RuntimeError where there is none."""
    hipcc = os.path.realpath(fbuild.find_hipcc())
    cand = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    if not os.path.exists(cand):
        raise RuntimeError(f"no clang++ beside {hipcc} ({cand})")
    return cand


def build_shim(out_dir, extra_flags=()) -> str:
    so = os.path.join(str(out_dir), "libweight_pack_shim.so")
    cmd = [find_clangxx(), "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", *extra_flags, SHIM, "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return so


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class Packer:
    """Every function returns the image as a uint16 array (halves) and its scale(s)."""

    def __init__(self, so_path):
        L = self.lib = ctypes.CDLL(so_path)
        fp, hp, i, lg = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint16), ctypes.c_int, ctypes.c_long
        for name, args, res in (("wp_split", [fp, i, i, i, hp, lg, fp], lg), ("wp_tiles", [fp, i, i, hp, lg, fp], lg),
                                ("wp_seq_attn", [fp, i, hp, lg, fp], lg), ("wp_seq_attn16", [fp, i, hp, lg, fp], lg),
                                ("wp_ffn16", [fp, fp, fp, i, i, hp, lg, hp, lg, ctypes.POINTER(lg), fp], lg),
                                ("wp_permuted_row", [i, i], i), ("wp_scale_for", [ctypes.c_float], ctypes.c_float),
                                ("wp_dense_bound", [fp, fp, i, i, i, ctypes.c_float], ctypes.c_float),
                                ("wp_ln_bound", [fp, fp, lg, ctypes.c_float, fp], None)):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, res

    @staticmethod
    def _buf(n):
        out = np.full(n, 0xFFFF, np.uint16)   # (a half the packer fails to write stays a NaN pattern)
        return out, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))

    def _one(self, fn, n_halves, *args):
        out, op = self._buf(n_halves)
        scale = ctypes.c_float(0)
        n = fn(*args, op, n_halves, ctypes.byref(scale))
        assert n == n_halves, (n, n_halves)
        return out, scale.value

    def split(self, W, row_pad=128):
        (N, K), (W, p) = np.shape(W), _f32(W)
        return self._one(self.lib.wp_split, -(-N // row_pad) * row_pad * K * 2, p, N, K, row_pad)

    def tiles(self, W):
        (N, K), (W, p) = np.shape(W), _f32(W)
        return self._one(self.lib.wp_tiles, -(-N // 384) * 384 * K * 2, p, N, K)

    def _attn(self, fn, W):
        d, (W, p) = np.shape(W)[1], _f32(W)
        assert W.shape == (3 * d, d)
        return self._one(fn, 6 * d * d, p, d)

    def seq_attn(self, W):
        return self._attn(self.lib.wp_seq_attn, W)

    def seq_attn16(self, W):
        return self._attn(self.lib.wp_seq_attn16, W)

    def ffn16(self, Wi, Wd, Wo=None):
        """-> plain stream, stream with attention.output.dense in front (None without Wo), (scale up, down, attention.output.dense)"""
        (ff, d), (Wi, pi), (Wd, pd) = np.shape(Wi), _f32(Wi), _f32(Wd)
        assert Wd.shape == (d, ff)
        Wo, po = _f32(Wo) if Wo is not None else (None, None)
        plain, pp = self._buf(4 * ff * d)
        tail, pt = self._buf(4 * ff * d + 2 * d * d if Wo is not None else 1)
        n_tail, scales = ctypes.c_long(-1), (ctypes.c_float * 3)()
        assert self.lib.wp_ffn16(pi, pd, po, d, ff, pp, plain.size, pt, tail.size, ctypes.byref(n_tail), scales) == plain.size
        assert n_tail.value == (tail.size if Wo is not None else 0)
        return plain, (tail if Wo is not None else None), tuple(scales)

    def permuted_row(self, i, j):
        return self.lib.wp_permuted_row(i, j)

    def scale_for(self, bound):
        return self.lib.wp_scale_for(ctypes.c_float(bound))

    def dense_bound(self, W, bias, r0, r1, in_l2):
        (W, pw), (bias, pb) = _f32(W), _f32(bias)
        return self.lib.wp_dense_bound(pw, pb, r0, r1, W.shape[1], ctypes.c_float(in_l2))

    def ln_bound(self, g, b, extra_each=0.0):
        (g, pg), (b, pb) = _f32(g), _f32(b)
        out = (ctypes.c_float * 2)()
        self.lib.wp_ln_bound(pg, pb, g.size, ctypes.c_float(extra_each), out)
        return out[0], out[1]


_packer = None


def load_packer(out_dir) -> Packer:
    """The packer of this process: the shim is built once, under the first `out_dir` asked for."""
    global _packer
    if _packer is None:
        _packer = Packer(build_shim(out_dir))
    return _packer


# ---- matrices whose packed halves identify their element.  An element is hi + lo with hi = code_hi and lo = code_lo, both exact
# fp16 values and their sum an exact fp32 value that rounds to hi: hi from the two fp16 binades [8192, 16384) (spacing 8) and
# [4096, 8192) (spacing 4), 0 < lo < 2 in steps of 2^-10.  The largest element lies in (8192, 16384), so the packer's scale is
# 2^shift for a matrix multiplied by 2^-shift (exact).  Coding "rc": hi names the row, lo the column; "cr": the other way round.
# Between them, the two packs make every half of an image name its (row, column).
MAX_CODE = 2046


def _hi_value(c):
    c = np.asarray(c) + 1                       # (8192 itself is left out: the largest element must lie above it)
    return np.where(c < 1024, 8192.0 + 8.0 * c, 4096.0 + 4.0 * (c - 1024))


def hi_code(v):
    """code of a packed hi half (float64 of the fp16 value); -1 for 0 (padding)"""
    v = np.asarray(v, np.float64)
    c = np.where(v >= 8192.0, (v - 8192.0) / 8.0, 1024 + (v - 4096.0) / 4.0) - 1
    return np.where(v == 0.0, -1, c)


def lo_code(v):
    v = np.asarray(v, np.float64)
    return np.where(v == 0.0, -1, v * 1024.0 - 1)


def coded(N, K, coding, shift=0):
    assert max(N, K) <= MAX_CODE + 1 and coding in ("rc", "cr")
    r, c = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    a, b = (r, c) if coding == "rc" else (c, r)
    xs = _hi_value(a) + (b + 1) / 1024.0
    w = (xs * 2.0 ** -shift).astype(np.float32)
    assert (w.astype(np.float64) * 2.0 ** shift == xs).all() and xs.max() > 8192.0
    return w


def halves(img):
    """the fp16 values of an image, as float64"""
    return np.asarray(img, np.uint16).view(np.float16).astype(np.float64)


def check_image(packer_fn, N, K, plane, row, col, shift=3):
    """Pack the two codings of an [N][K] matrix with `packer_fn(W) -> (image, scale)` and compare every half with the expected
    (plane, row, col) arrays (one entry per half; row = -1: padding, the half is zero)."""
    plane, row, col = (np.asarray(a).reshape(-1) for a in (plane, row, col))
    for coding in ("rc", "cr"):
        img, scale = packer_fn(coded(N, K, coding, shift))
        assert scale == 2.0 ** shift, (coding, scale)
        v = halves(img)
        assert v.shape == plane.shape, (v.shape, plane.shape)
        pad = row < 0
        assert (v[pad] == 0).all()
        want_hi, want_lo = (row, col) if coding == "rc" else (col, row)
        hi, lo = (plane == 0) & ~pad, (plane == 1) & ~pad
        assert (hi | lo | pad).all()
        assert (hi_code(v[hi]) == want_hi[hi]).all(), coding
        assert (lo_code(v[lo]) == want_lo[lo]).all(), coding


# ---- the ffn16 stream's consumption order (ffn16.hip: what tests/test_host.py derives from the kernel's step calls)
def ffn16_consumed(nkt, ng, tail):
    """("ao", local step) | ("up" | "down", group, local step) per stream step: attention.output.dense (nkt^2 / 2 steps, TAIL only) | up(0) | up(1) down(0) |
    ... | up(ng - 1) down(ng - 2) | down(ng - 1)"""
    out = [("ao", s) for s in range(nkt * nkt // 2 if tail else 0)] + [("up", 0, s) for s in range(nkt)]
    for G in range(ng):
        if G + 1 < ng:
            out += [("up", G + 1, s) for s in range(nkt)]
        out += [("down", G, s) for s in range(nkt)]
    return out


def ffn16_steps(stream):
    """a stream as [step][tile 0-3][unit 0-7][row 0-15][8 halves] fp16 values (float64)"""
    return halves(stream).reshape(-1, 4, 8, 16, 8)


def ffn16_step_ids(packer, d, ff, tail):
    """What the packed stream holds, step by step, read off the REAL bytes: ("ao", local step) | ("up", group, local step) |
    ("down", group, local step).  One matrix at a time is coded (hi = row, lo = column) and the other two are zero, so a step's
    non-zero halves say whose it is; all 4096 halves of a step must then name the 64 weight rows and the 32 columns of exactly one
    (block, step): up(G) step ks = features 64 G .. + 63, k32 step ks; down(G) step pr * (d / 64) + q = output features 64 q .. + 63
    (output tiles 4 q .. 4 q + 3), k32 step 2 G + pr; attention.output.dense step kt * (d / 64) + q likewise with k32 step kt."""
    nkt = d // 32
    mats = {"up": coded(ff, d, "rc", 3), "down": coded(d, ff, "rc", 3), "ao": coded(d, d, "rc", 3)}
    ids = {}
    for blk in ("up", "down", "ao") if tail else ("up", "down"):
        Wi, Wd, Wo = (mats[b] if b == blk else 0 * mats[b] for b in ("up", "down", "ao"))
        plain, with_tail, _ = packer.ffn16(Wi, Wd, Wo if tail else None)
        steps = ffn16_steps(with_tail if tail else plain)
        for p in np.flatnonzero(steps.reshape(len(steps), -1).any(axis=1)):
            assert steps[p].all() and p not in ids, (blk, p)
            rows, cols = hi_code(steps[p][:, :4]), lo_code(steps[p][:, 4:])
            r0, c0 = int(rows.min()), int(cols.min())
            assert r0 % 64 == 0 and c0 % 32 == 0
            assert sorted(set(rows.reshape(-1))) == list(range(r0, r0 + 64)) and sorted(set(cols.reshape(-1))) == list(range(c0, c0 + 32))
            if blk == "up":
                ids[p] = ("up", r0 // 64, c0 // 32)
            elif blk == "down":
                ids[p] = ("down", c0 // 64, (c0 // 32) % 2 * (nkt // 2) + r0 // 64)
            else:
                ids[p] = ("ao", (c0 // 32) * (nkt // 2) + r0 // 64)
    assert sorted(ids) == list(range(len(steps)))
    return [ids[p] for p in range(len(steps))]


# ---- the fixed inputs of the golden hashes
def weights(seed, N, K, std=0.02):
    return (np.random.RandomState(seed).randn(N, K) * std).astype(np.float32)


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def record_all(packer):
    """{image name: {"sha256": ..., "halves": ..., "scale": ... | "scales": [...]}} for every layout at every shape of SHAPES, and the
    special inputs."""
    out = {}

    def one(name, res):
        img, scale = res
        out[name] = {"sha256": sha(img), "halves": int(img.size), "scale": float(scale)}

    for d, ff in SHAPES:
        tag = f"d{d}_ff{ff}"
        wqkv, wo, wi, wd = weights(d, 3 * d, d), weights(d + 1, d, d), weights(d + 2, ff, d), weights(d + 3, d, ff, 0.015)
        one(f"{tag}/split_wo", packer.split(wo))
        one(f"{tag}/tiles_wqkv", packer.tiles(wqkv))
        one(f"{tag}/tiles_wqk", packer.tiles(wqkv[:2 * d]))
        one(f"{tag}/tiles_wv", packer.tiles(wqkv[2 * d:]))
        one(f"{tag}/tiles_wo", packer.tiles(wo))
        one(f"{tag}/tiles_wi", packer.tiles(wi))
        one(f"{tag}/tiles_wd", packer.tiles(wd))
        one(f"{tag}/seq_attn", packer.seq_attn(wqkv))
        one(f"{tag}/seq_attn16", packer.seq_attn16(wqkv))
        plain, tail, scales = packer.ffn16(wi, wd, wo)
        out[f"{tag}/ffn16"] = {"sha256": sha(plain), "halves": int(plain.size), "scales": [float(s) for s in scales[:2]]}
        out[f"{tag}/ffn16_tail"] = {"sha256": sha(tail), "halves": int(tail.size), "scales": [float(s) for s in scales]}
        plain2, none, scales2 = packer.ffn16(wi, wd)
        assert none is None and (plain2 == plain).all() and scales2[:2] == scales[:2]
    one("demb_63x32_pad128", packer.split(weights(7, 63, 32, 0.05), 128))
    one("tiles_100x64", packer.tiles(weights(8, 100, 64)))
    one("zero/split", packer.split(np.zeros((96, 64), np.float32)))
    one("zero/tiles", packer.tiles(np.zeros((96, 64), np.float32)))
    mixed = weights(9, 128, 64, 1.0)
    mixed[::2, 1::2] *= 1e-9     # entries near 1e-9 beside entries near 1: their lo halves are subnormal or zero
    one("mixed_1e-9/split", packer.split(mixed))
    one("mixed_1e-9/tiles", packer.tiles(mixed))
    return out
