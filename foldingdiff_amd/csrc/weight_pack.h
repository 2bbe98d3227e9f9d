// The weight packer: fp32 weight matrices -> the fp16 hi | lo byte images the row-image kernels stream straight into LDS, and the
// static power-of-two scales of the activation images.  Arithmetic on host arrays only -- no HIP, no model -- so that it runs
// (and is tested byte by byte, tests/test_weight_pack.py) without a GPU.  api_weights.hip uploads what these functions return.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace fdmi {

// an image in halves (uint16_t = the bits of an fp16) with  w * scale = hi + lo
struct Image {
  std::vector<uint16_t> data;
  float scale = 1.f;
};

// W [N][K] fp32 -> [N padded to row_pad][K/32][hi x32 | lo x32] fp16 with w*scale = hi + lo (img_common.h).
// scale = the power of two that puts max|w|*scale in [8192, 16384): every lo of a weight that
// matters is a normal fp16 and nothing overflows.  A block [hi x32 | lo x32] = eight 16-byte units: 0-3 hi of k 8 u .. 8 u + 7, 4-7 lo.
inline Image pack_split_weight(const float* W, int N, int K, int row_pad = 128) {
  Image im;
  float mx = 0.f;
  for (size_t i = 0; i < (size_t)N * K; ++i) mx = std::fmax(mx, std::fabs(W[i]));
  if (mx > 0.f && std::isfinite(mx)) im.scale = std::exp2(std::floor(std::log2(16384.0f / mx)));
  const float s = im.scale;
  const int npad = (N + row_pad - 1) / row_pad * row_pad, nk = K / 32;
  im.data.assign((size_t)npad * nk * 64, 0);
  for (int n = 0; n < N; ++n)
    for (int kt = 0; kt < nk; ++kt) {
      uint16_t* dst = im.data.data() + ((size_t)n * nk + kt) * 64;
      for (int j = 0; j < 32; ++j) {
        const float xs = W[(size_t)n * K + kt * 32 + j] * s;
        const _Float16 hi = (_Float16)xs;
        const _Float16 lo = (_Float16)(xs - (float)hi);
        memcpy(dst + j, &hi, 2);
        memcpy(dst + 32 + j, &lo, 2);
      }
    }
  return im;
}

// Row-image GEMM weights, ordered [384-row tile][k-tile][48 KiB = the workgroup's LDS stage, byte for byte]: the loader copies a
// k-tile with lane-linear LDS-DMA from CONSECUTIVE cache lines.  The stage is 48 pieces of 8 rows, each piece unit-major:
// [piece j][position p][row % 8][16 B] with position p holding 16-byte unit p ^ (j & 1) of the row's block (the layout the
// compute waves' fragment reads are bank-conflict free on; gemm_img.hip uses the same for the activation pieces).
// Rows padded to whole tiles with zeros.
inline Image pack_weight_tiles(const float* W, int N, int K) {
  const Image rm = pack_split_weight(W, N, K, 384);
  Image im{std::vector<uint16_t>(rm.data.size(), 0), rm.scale};
  const int npad = (N + 383) / 384 * 384, nk = K / 32;
  for (int n = 0; n < npad; ++n)
    for (int kt = 0; kt < nk; ++kt) {
      const int R = n % 384, j = R >> 3, r = R & 7;
      uint16_t* stage = im.data.data() + ((size_t)(n / 384) * nk + kt) * 384 * 64;
      const uint16_t* blk = rm.data.data() + ((size_t)n * nk + kt) * 64;
      for (int u = 0; u < 8; ++u) memcpy(stage + (j * 1024 + (((u ^ (j & 1)) * 8 + r) << 4)) / 2, blk + u * 8, 16);
    }
  return im;
}

// seq_attn.hip's weights: the q | k | v projection W [3 d][d] ordered per head, [head][k-tile][unit 0-7][96 rows: q_h | k_h | v_h][16 B]
// (a k-tile of a head = one 12 KiB LDS ring stage, byte for byte, unit-major), split at ONE scale for the whole matrix -- the scale
// of the tile image of the same matrix -- so the fused kernel multiplies the very same fp16 hi / lo values as the tile GEMM.
inline Image pack_seq_attn(const float* W, int d) {
  const Image rm = pack_split_weight(W, 3 * d, d, 384);
  const int nk = d / 32, H = d / 32;
  Image im{std::vector<uint16_t>((size_t)H * nk * 96 * 64, 0), rm.scale};
  for (int h = 0; h < H; ++h)
    for (int kt = 0; kt < nk; ++kt) {
      uint16_t* stage = im.data.data() + ((size_t)h * nk + kt) * 96 * 64;
      for (int r = 0; r < 96; ++r) {
        const int n = (r / 32) * d + h * 32 + (r % 32);
        const uint16_t* blk = rm.data.data() + ((size_t)n * nk + kt) * 64;
        for (int u = 0; u < 8; ++u) memcpy(stage + ((size_t)u * 96 + r) * 8, blk + u * 8, 16);
      }
    }
  return im;
}

// ---- operand tiles of v_mfma_f32_16x16x32_f16 (seq_attn16.hip, ffn16.hip): 16 rows of one k32 step, unit-major
// [unit 0-7][row 0-15][16 B] = 2 KiB.  Row i of the j-th tile of a pair holds feature 8 (i / 4) + 4 j + (i % 4) of the pair's 32:
// with that order the 16 x 16 C/D layout gives every lane eight consecutive features of its token, which is exactly its operand
// unit of the next contraction (ffn16.hip).
inline int permuted_row(int i, int j) { return 8 * (i / 4) + 4 * j + (i % 4); }

// the tile whose row i is row  row0 + permuted_row(i, j)  of the row-major split image rm ([rows][nk][64 halves]), k32 step kt
inline void put_tile(uint16_t* tile, const uint16_t* rm, int nk, int row0, int j, int kt) {
  for (int i = 0; i < 16; ++i) {
    const uint16_t* blk = rm + ((size_t)(row0 + permuted_row(i, j)) * nk + kt) * 64;
    for (int u = 0; u < 8; ++u) memcpy(tile + ((size_t)u * 16 + i) * 8, blk + u * 8, 16);
  }
}

// seq_attn16.hip's weights: [head][k32 step][tile: q 0, q 1, k 0, k 1, v 0, v 1][unit 0-7][row 0-15][16 B] (a k32 step of a head = 12 KiB,
// two of them = one LDS ring stage byte for byte).  Split at the SAME scale as pack_seq_attn.
inline Image pack_seq_attn16(const float* W, int d) {
  const Image rm = pack_split_weight(W, 3 * d, d, 384);
  const int nk = d / 32, H = d / 32;
  Image im{std::vector<uint16_t>((size_t)H * nk * 96 * 64, 0), rm.scale};
  for (int h = 0; h < H; ++h)
    for (int kt = 0; kt < nk; ++kt)
      for (int t = 0; t < 6; ++t)
        put_tile(im.data.data() + (((size_t)h * nk + kt) * 6 + t) * 1024, rm.data.data(), nk, (t >> 1) * d + h * 32, t & 1, kt);
  return im;
}

// ffn16.hip's weights: intermediate.dense Wi [ff][d] and output.dense Wd [d][ff] as ONE stream in consumption order.  Per group G of 64
// intermediate features (the first dense runs one group ahead of the second: up(0) | up(1) down(0) | ... | up(ng - 1) down(ng - 2) |
// down(ng - 1)): d / 32 steps of the first dense (k32 step ks: four tiles, tile t = 2 pair + j, row i = feature
// 64 G + 32 pair + permuted_row(i, j)), then d / 32 steps of the second (pair 0, 1: its 32 features are one k32 step; output
// tiles T = 0 .. d / 16 - 1 four to a step, tile T = 2 kt + j, row i = output feature 32 kt + permuted_row(i, j)).  A step = four
// tiles = 8 KiB, two steps = one LDS ring stage byte for byte.  Each matrix is split at its own power-of-two scale.
// `tail` (Wo non-null) is the same stream with attention.output.dense Wo [d][d] in front (ffn16.hip TAIL): step kt * (d / 64) + q =
// k32 step kt of the context against the output tiles 4 q .. 4 q + 3 (rows permuted like the second dense's).
struct Ffn16Images {
  Image plain, tail;     // plain.scale = intermediate.dense's, tail.scale = attention.output.dense's (tail.data empty without Wo)
  float scale_dn = 1.f;  // output.dense's
};
inline Ffn16Images pack_ffn16(const float* Wi, const float* Wd, const float* Wo, int d, int ff) {
  Ffn16Images out;
  const Image ri = pack_split_weight(Wi, ff, d, 128), rd = pack_split_weight(Wd, d, ff, 128);
  out.plain.scale = ri.scale;
  out.scale_dn = rd.scale;
  const int nkt = d / 32, ng = ff / 64, spg = 2 * nkt, nkd = ff / 32;
  constexpr size_t kStep = 4 * 1024;  // halves
  // the d / 16 output tiles of k32 step kt of a dense rm [d][nk * 32], four to a step
  auto put_out_tiles = [&](uint16_t* steps, const Image& rm, int nk, int kt) {
    for (int T = 0; T < 2 * nkt; ++T) put_tile(steps + (size_t)T * 1024, rm.data.data(), nk, 32 * (T >> 1), T & 1, kt);
  };
  out.plain.data.assign((size_t)ng * spg * kStep, 0);
  uint16_t* const plain = out.plain.data.data();
  // stream position (in steps) of a group's blocks: up(0) | up(1) down(0) | up(2) down(1) | ... | up(ng - 1) down(ng - 2) | down(ng - 1)
  auto up_at = [&](int G) { return G == 0 ? 0 : nkt + (G - 1) * spg; };
  auto down_at = [&](int G) { return G == ng - 1 ? nkt + (ng - 1) * spg : nkt + G * spg + nkt; };
  for (int G = 0; G < ng; ++G) {
    for (int ks = 0; ks < nkt; ++ks)
      for (int t = 0; t < 4; ++t)
        put_tile(plain + (up_at(G) + ks) * kStep + (size_t)t * 1024, ri.data.data(), nkt, 64 * G + 32 * (t >> 1), t & 1, ks);
    for (int pr = 0; pr < 2; ++pr) put_out_tiles(plain + (down_at(G) + pr * (nkt / 2)) * kStep, rd, nkd, 2 * G + pr);
  }
  if (Wo) {
    const Image ro = pack_split_weight(Wo, d, d, 128);
    out.tail.scale = ro.scale;
    const size_t nsa = (size_t)nkt * nkt / 2;
    out.tail.data.assign(nsa * kStep + out.plain.data.size(), 0);
    for (int kt = 0; kt < nkt; ++kt) put_out_tiles(out.tail.data.data() + (size_t)kt * (nkt / 2) * kStep, ro, nkt, kt);
    memcpy(out.tail.data.data() + nsa * kStep, plain, out.plain.data.size() * 2);
  }
  return out;
}

// ---- static scales of the activation images (row-image path).
// Every image tensor gets the largest power of two s with  bound * s <= 30000 < fp16 max, where `bound` is a
// guaranteed bound of |x| derived from the weights: a LayerNorm output obeys |y_i| <= max|gamma| sqrt(d) + max|beta|
// and ||y||_2 <= max|gamma| sqrt(d) + ||beta||_2; a dense output |y W_j + b_j| <= ||y||_2 ||W_j||_2 + |b_j|; GELU and the
// softmax-weighted average of V do not grow their argument.  Nothing overflows for ANY weights (trained outliers
// included); elements far below the bound merely lose low bits of `lo` (absolute error bound * 2^-40).
inline float scale_for(float bound) {
  if (!(bound > 0.f) || !std::isfinite(bound)) return 1.f;
  float e = std::floor(std::log2(30000.0f / bound));
  e = e < -40.f ? -40.f : (e > 40.f ? 40.f : e);
  return std::exp2(e);
}

struct Bound {
  float linf, l2;
};
// bound of a LayerNorm's outputs (gamma g, beta b, d features), each raised by extra_each
inline Bound ln_bound(const float* g, const float* b, size_t d, float extra_each = 0.f) {
  float gm = 0.f, bm = 0.f;
  double b2 = 0.0;
  for (size_t i = 0; i < d; ++i) {
    gm = std::fmax(gm, std::fabs(g[i]));
    bm = std::fmax(bm, std::fabs(b[i]));
    b2 += (double)b[i] * b[i];
  }
  const float sd = std::sqrt((float)d);
  return Bound{gm * sd + bm + extra_each, gm * sd + (float)std::sqrt(b2) + extra_each * sd};
}

// bound of a dense layer's outputs (rows [r0, r1) of W [N][K]) for inputs with ||x||_2 <= in_l2
inline float dense_bound(const float* W, const float* bias, int r0, int r1, int K, float in_l2) {
  float worst = 0.f;
  for (int j = r0; j < r1; ++j) {
    double n2 = 0.0;
    for (int k = 0; k < K; ++k) n2 += (double)W[(size_t)j * K + k] * W[(size_t)j * K + k];
    worst = std::fmax(worst, (float)std::sqrt(n2) * in_l2 + std::fabs(bias[j]));
  }
  return worst;
}

}  // namespace fdmi
