// A stand-alone run of the weight packer (csrc/weight_pack.h) under AddressSanitizer and UndefinedBehaviorSanitizer: every
// layout at (d_model, d_ff) = (64, 128), (192, 384), (384, 768), the distance table at 63 x 32, a tile image with padding rows
// inside a tile (100 x 64), an all-zero matrix and one with entries near 1e-9 beside entries near 1.  Host only, no GPU:
//
//   <rocm>/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/weight_pack_sanitize.cpp -o weight_pack_sanitize && ./weight_pack_sanitize
//
// Exit status 0 and "ok" = no finding.  (Not part of the pytest suite, and never loaded into Python.)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../foldingdiff_amd/csrc/weight_pack.h"

namespace {
uint32_t g_state = 12345u;
float unit() {  // uniform in [-1, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 8388608.0f - 1.0f;
}
std::vector<float> matrix(int N, int K, float amp) {
  std::vector<float> w((size_t)N * K);
  for (float& v : w) v = unit() * amp;
  return w;
}
size_t g_halves = 0;
uint64_t g_sum = 0;
void eat(const std::vector<uint16_t>& img) {  // reads every half, so that an image shorter than its loops claim is found
  g_halves += img.size();
  for (uint16_t h : img) g_sum += h;
}
}  // namespace

int main() {
  using namespace fdmi;
  const int shapes[3][2] = {{64, 128}, {192, 384}, {384, 768}};
  for (const auto& s : shapes) {
    const int d = s[0], ff = s[1];
    const std::vector<float> wqkv = matrix(3 * d, d, 0.06f), wo = matrix(d, d, 0.06f), wi = matrix(ff, d, 0.06f), wd = matrix(d, ff, 0.04f);
    const std::vector<float> bias = matrix(3 * d, 1, 0.1f), g = matrix(d, 1, 1.0f), b = matrix(d, 1, 0.3f);
    eat(pack_split_weight(wo.data(), d, d).data);
    eat(pack_weight_tiles(wqkv.data(), 3 * d, d).data);
    eat(pack_weight_tiles(wqkv.data(), 2 * d, d).data);
    eat(pack_weight_tiles(wqkv.data() + (size_t)2 * d * d, d, d).data);
    eat(pack_weight_tiles(wi.data(), ff, d).data);
    eat(pack_weight_tiles(wd.data(), d, ff).data);
    eat(pack_seq_attn(wqkv.data(), d).data);
    eat(pack_seq_attn16(wqkv.data(), d).data);
    const Ffn16Images with_tail = pack_ffn16(wi.data(), wd.data(), wo.data(), d, ff), plain = pack_ffn16(wi.data(), wd.data(), nullptr, d, ff);
    eat(with_tail.plain.data);
    eat(with_tail.tail.data);
    eat(plain.plain.data);
    if (!plain.tail.data.empty() || plain.plain.data != with_tail.plain.data) return 2;
    const Bound hb = ln_bound(g.data(), b.data(), (size_t)d, 1.0f);
    if (!(scale_for(hb.linf) > 0.f) || !(scale_for(dense_bound(wqkv.data(), bias.data(), d, 2 * d, d, hb.l2)) > 0.f)) return 3;
  }
  eat(pack_split_weight(matrix(63, 32, 0.1f).data(), 63, 32, 128).data);
  eat(pack_weight_tiles(matrix(100, 64, 0.06f).data(), 100, 64).data);
  const std::vector<float> zero((size_t)96 * 64, 0.f);
  const Image z = pack_weight_tiles(zero.data(), 96, 64);
  eat(z.data);
  if (z.scale != 1.f || g_sum == 0) return 4;
  std::vector<float> mixed = matrix(128, 64, 1.0f);
  for (size_t i = 0; i < mixed.size(); i += 3) mixed[i] *= 1e-9f;
  eat(pack_split_weight(mixed.data(), 128, 64).data);
  eat(pack_weight_tiles(mixed.data(), 128, 64).data);
  std::printf("ok: %zu halves packed (checksum %llu)\n", g_halves, (unsigned long long)g_sum);
  return 0;
}
