"""csrc/weight_pack.h, the real packer, on the CPU (through tests/weight_pack_shim.cpp, built here with the ROCm clang++):
(a) the bytes of every image for fixed inputs against tests/golden/weight_images.json; (b) every 16-byte unit of every layout
against the layout's stated contract, by value, on matrices whose packed halves name their (row, column); (c) the scale rules."""
import json

import numpy as np
import pytest

import weight_pack_cases as cases
from weight_pack_cases import check_image, coded, halves, hi_code, lo_code


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    try:
        cases.find_clangxx()
    except RuntimeError as e:
        pytest.skip(str(e))
    return cases.load_packer(tmp_path_factory.mktemp("weight_pack"))


def perm(i, j):
    """row i of the j-th tile of a pair holds feature 8 (i / 4) + 4 j + (i % 4) of the pair's 32"""
    return 8 * (i // 4) + 4 * j + (i % 4)


# ---- (a) bytes unchanged
def test_image_bytes_match_the_golden_hashes(packer):
    with open(cases.GOLDEN) as fh:
        want = json.load(fh)
    got = cases.record_all(packer)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    assert want["zero/split"]["scale"] == 1.0 and want["zero/tiles"]["scale"] == 1.0


def test_zero_and_tiny_entries(packer):
    """an all-zero matrix: scale 1 and a zero image; entries near 1e-9 beside entries near 1: hi + lo still is the nearest the
    format allows, and some lo halves are subnormal or zero"""
    for fn in (packer.split, packer.tiles):
        img, scale = fn(np.zeros((96, 64), np.float32))
        assert scale == 1.0 and not img.any()
    w = cases.weights(9, 128, 64, 1.0)
    w[::2, 1::2] *= 1e-9
    img, scale = packer.split(w)
    v = halves(img).reshape(128, 2, 2, 32)                 # [row][k-tile][hi | lo][32]
    hi, lo = v[:, :, 0].reshape(128, 64), v[:, :, 1].reshape(128, 64)
    small = np.abs(lo) < 2.0 ** -14
    assert small[::2, 1::2].all() and (lo[::2, 1::2] == 0).any() and not small[1::2].all()
    # scaled, a tiny entry is about 1e-5: hi carries it to 2^-11 relative and lo (a subnormal: steps of 2^-24) to 2^-25 absolute
    err = np.abs((hi + lo) / scale - w.astype(np.float64))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(w), 2.0 ** -25 / scale)).all()


@pytest.mark.parametrize("N,K,row_pad", [(63, 32, 128), (100, 64, 384), (192, 192, 128)])
def test_row_major_split_is_hi_plus_lo_of_the_scaled_weight(packer, N, K, row_pad):
    """[row padded to row_pad][k-tile][hi x32 | lo x32], hi = fp16(w s), lo = fp16(w s - hi), s = the power of two that puts
    max|w| s in [8192, 16384); bit for bit against numpy's fp16 rounding (round to nearest even, like _Float16's)"""
    w = cases.weights(N + K, N, K)
    img, scale = packer.split(w, row_pad)
    mx = np.abs(w).max()
    assert 8192.0 <= mx * scale < 16384.0 and np.log2(scale) == np.floor(np.log2(scale))
    xs = w * np.float32(scale)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    npad = -(-N // row_pad) * row_pad
    want = np.zeros((npad, K // 32, 2, 32), np.float16)
    want[:N, :, 0] = hi.reshape(N, K // 32, 32)
    want[:N, :, 1] = lo.reshape(N, K // 32, 32)
    assert (img == want.reshape(-1).view(np.uint16)).all()
    check_image(lambda W: packer.split(W, row_pad), N, K,
                *np.broadcast_arrays(*_block_ids(npad, N, K)))


def _block_ids(npad, N, K):
    """(plane, row, col) of the row-major split image [npad][K / 32][hi | lo][32]"""
    n, kt, pl, j = np.ogrid[:npad, :K // 32, :2, :32]
    return pl, np.where(n < N, n, -1), 32 * kt + j


# ---- (b) each layout against its stated contract
@pytest.mark.parametrize("N,K", [(100, 64), (384, 384), (768, 384), (1152, 384), (384, 768), (400, 32)])
def test_tile_stage_layout(packer, N, K):
    """[384-row tile][k-tile][piece 0-47][position 0-7][row % 8][16 B]: unit u of row R sits in piece R / 8 at position u ^ (piece & 1),
    at row R % 8; unit u = plane u / 4 (hi | lo), k 8 (u % 4) .. + 7 of the k-tile; rows beyond N are zero"""
    T, kt, j, p, r, e = np.ogrid[:-(-N // 384), :K // 32, :48, :8, :8, :8]
    u = p ^ (j & 1)
    n = 384 * T + 8 * j + r
    check_image(packer.tiles, N, K, *np.broadcast_arrays(u // 4, np.where(n < N, n, -1), 32 * kt + 8 * (u % 4) + e))


@pytest.mark.parametrize("d", [64, 192, 384])
def test_seq_attn_stage_layout_through_the_fragment_reads(packer, d):
    """[head][k-tile][12 KiB stage]; seq_attn.hip's rd_w: lane (l31, half) reads 16 bytes at stage + (unit + half) * 1536 + j * 512 +
    l31 * 16 for accumulator j, unit = 2 c + 4 plane, and must get W[j d + 32 head + l31][32 kt + 16 c + 8 half + 0..7] of the plane.
    The reads of a stage cover it exactly once."""
    H = nk = d // 32
    plane, row, col = (np.full((H, nk, 6144), -2) for _ in range(3))
    h, kt, j, l31, half, unit, e = np.ogrid[:H, :nk, :3, :32, :2, :8:2, :8]      # unit 0, 2, 4, 6
    at = ((unit + half) * 1536 + j * 512 + l31 * 16) // 2 + e
    hh, kk, at = np.broadcast_arrays(h, kt, at)
    for dst, val in ((plane, unit // 4), (row, j * d + 32 * h + l31), (col, 32 * kt + 16 * ((unit % 4) // 2) + 8 * half + e)):
        dst[hh, kk, at] = np.broadcast_to(val, at.shape)
    assert at.size == plane.size and (plane >= 0).all()
    check_image(packer.seq_attn, 3 * d, d, plane, row, col)


@pytest.mark.parametrize("d", [64, 192, 384])
def test_seq_attn16_tile_layout(packer, d):
    """[head][k32 step][tile q0 q1 k0 k1 v0 v1][unit 0-7][row 0-15][16 B]: row i of tile j of a pair holds head feature
    8 (i / 4) + 4 j + (i % 4)"""
    assert [packer.permuted_row(i, j) for j in range(2) for i in range(16)] == [perm(i, j) for j in range(2) for i in range(16)]
    H = nk = d // 32
    h, kt, t, u, i, e = np.ogrid[:H, :nk, :6, :8, :16, :8]
    check_image(packer.seq_attn16, 3 * d, d, *np.broadcast_arrays(u // 4, (t // 2) * d + 32 * h + perm(i, t % 2), 32 * kt + 8 * (u % 4) + e))
    # and the scale is the tile image's and seq_attn's: the fused kernels multiply the same halves as the tile GEMM
    w = cases.weights(d, 3 * d, d)
    assert packer.seq_attn16(w)[1] == packer.seq_attn(w)[1] == packer.tiles(w)[1]


def ffn16_expected(d, ff, tail):
    """(matrix 0 Wi | 1 Wd | 2 Wo, plane, row, col) per half of the stream [step][tile 0-3][unit 0-7][row 0-15][8], from the order in
    which the kernel consumes steps (cases.ffn16_consumed) and the tile contract of each block: attention.output.dense step
    kt * (d / 64) + q = k32 step kt against output tiles 4 q .. 4 q + 3; up(G) step ks = k32 step ks, tile t = features
    64 G + 32 (t / 2) + perm(i, t % 2); down(G) step pr * (d / 64) + q = k32 step 2 G + pr against output tiles 4 q .. 4 q + 3;
    output tile T = features 32 (T / 2) + perm(i, T % 2)"""
    nkt, ng = d // 32, ff // 64
    consumed = cases.ffn16_consumed(nkt, ng, tail)
    mat, row, k32 = (np.zeros((len(consumed), 4, 1, 16, 1), np.int64) for _ in range(3))
    t, i = np.arange(4).reshape(4, 1, 1, 1), np.arange(16).reshape(1, 1, 16, 1)
    for p, (blk, *G, s) in enumerate(consumed):
        G = G[0] if G else 0
        if blk == "up":
            mat[p], row[p], k32[p] = 0, 64 * G + 32 * (t // 2) + perm(i, t % 2), s
        else:
            T = 4 * (s % (nkt // 2)) + t
            mat[p], row[p] = (1 if blk == "down" else 2), 32 * (T // 2) + perm(i, T % 2)
            k32[p] = 2 * G + s // (nkt // 2) if blk == "down" else s // (nkt // 2)
    u, e = np.arange(8).reshape(1, 1, 8, 1, 1), np.arange(8).reshape(1, 1, 1, 1, 8)
    return [a.reshape(-1) for a in np.broadcast_arrays(mat, u // 4, row, 32 * k32 + 8 * (u % 4) + e)]


@pytest.mark.parametrize("d,ff", cases.SHAPES)
def test_ffn16_stream_layout(packer, d, ff):
    """the stream with and without attention.output.dense in front, every half by value; the tail stream's back part equals the
    plain stream byte for byte; each matrix at its own scale"""
    shifts = (3, 5, 7)
    for coding in ("rc", "cr"):
        Wi, Wd, Wo = coded(ff, d, coding, shifts[0]), coded(d, ff, coding, shifts[1]), coded(d, d, coding, shifts[2])
        plain, tail, scales = packer.ffn16(Wi, Wd, Wo)
        assert scales == tuple(2.0 ** s for s in shifts)
        plain_alone, none, scales_alone = packer.ffn16(Wi, Wd)
        assert none is None and (plain_alone == plain).all() and scales_alone[:2] == scales[:2]
        assert tail.size == plain.size + 2 * d * d and (tail[2 * d * d:] == plain).all()
        for img, has_tail in ((plain, False), (tail, True)):
            mat, plane, row, col = ffn16_expected(d, ff, has_tail)
            v = halves(img)
            assert v.shape == mat.shape
            want_hi, want_lo = (row, col) if coding == "rc" else (col, row)
            assert (hi_code(v[plane == 0]) == want_hi[plane == 0]).all() and (lo_code(v[plane == 1]) == want_lo[plane == 1]).all()
        # which matrix a half belongs to: with the other two zero, exactly its halves are non-zero (a coded half never is zero)
        mat = ffn16_expected(d, ff, True)[0]
        for m, only in enumerate(((Wi, 0 * Wd, 0 * Wo), (0 * Wi, Wd, 0 * Wo), (0 * Wi, 0 * Wd, Wo))):
            assert ((halves(packer.ffn16(*only)[1]) != 0) == (mat == m)).all(), m


# ---- (c) the scale rules
def test_scale_for_matches_its_restatement(packer):
    f32 = np.float32

    def scale_for(bound):                       # tests/test_host.py: test_f16x3_split_arithmetic_is_fp32_class
        return f32(2.0 ** np.clip(np.floor(np.log2(30000.0 / bound)), -40, 40))

    for bound in (0.0, -1.0, -np.inf, np.nan, np.inf):
        assert packer.scale_for(bound) == 1.0, bound
    bounds = [1e-30, 1e30, 1.0, 3.7, 29999.0, 30000.0, 30001.0] + [2.0 ** k for k in range(-50, 51)] + [30000.0 / 2.0 ** k for k in range(-45, 46)]
    assert 2.0 ** 14 in bounds and 2.0 ** 15 in bounds      # the powers of two on both sides of 30000
    for bound in bounds:
        b = float(f32(bound))
        got = packer.scale_for(b)
        assert got == scale_for(b), (bound, got)
        assert 2.0 ** -40 <= got <= 2.0 ** 40
        if 2.0 ** -39 < got < 2.0 ** 40:
            assert b * got <= 30000.0 < 2 * b * got, bound      # the largest power of two with bound * s <= 30000
    assert packer.scale_for(1e-30) == 2.0 ** 40 and packer.scale_for(1e30) == 2.0 ** -40


def test_dense_and_layernorm_bounds_against_float64(packer):
    d, ff = 64, 128
    rng = np.random.RandomState(3)
    W, bias = (rng.randn(ff, d) * 0.05).astype(np.float32), (rng.randn(ff) * 0.1).astype(np.float32)
    W64, b64 = W.astype(np.float64), bias.astype(np.float64)
    for r0, r1, in_l2 in ((0, ff, 9.5), (d, ff, 1.0), (5, 6, 0.0)):
        want = (np.sqrt((W64[r0:r1] ** 2).sum(1)) * in_l2 + np.abs(b64[r0:r1])).max()
        assert packer.dense_bound(W, bias, r0, r1, in_l2) == pytest.approx(want, rel=4 * 2.0 ** -24)
    g, b = (1.0 + rng.randn(d) * 0.2).astype(np.float32), (rng.randn(d) * 0.3).astype(np.float32)
    g64, b64 = np.abs(g.astype(np.float64)), b.astype(np.float64)
    for extra in (0.0, 1.0):
        linf, l2 = packer.ln_bound(g, b, extra)
        assert linf == pytest.approx(g64.max() * 8.0 + np.abs(b64).max() + extra, rel=4 * 2.0 ** -24)
        assert l2 == pytest.approx(g64.max() * 8.0 + np.sqrt((b64 ** 2).sum()) + extra * 8.0, rel=4 * 2.0 ** -24)
