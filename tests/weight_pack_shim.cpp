// C wrappers around csrc/weight_pack.h for tests/test_weight_pack.py (host-only; built by the test, loaded with ctypes).
// An image goes to a caller-provided buffer of `cap` halves; the return value is the image's length in halves, negated
// when the buffer is too small (nothing is written then).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../foldingdiff_amd/csrc/weight_pack.h"

namespace {
long give(const std::vector<uint16_t>& img, uint16_t* out, long cap) {
  const long n = (long)img.size();
  if (n > cap) return -n;
  std::copy(img.begin(), img.end(), out);
  return n;
}
long give(const fdmi::Image& im, uint16_t* out, long cap, float* scale) {
  *scale = im.scale;
  return give(im.data, out, cap);
}
}  // namespace

extern "C" {

long wp_split(const float* W, int N, int K, int row_pad, uint16_t* out, long cap, float* scale) {
  return give(fdmi::pack_split_weight(W, N, K, row_pad), out, cap, scale);
}
long wp_tiles(const float* W, int N, int K, uint16_t* out, long cap, float* scale) {
  return give(fdmi::pack_weight_tiles(W, N, K), out, cap, scale);
}
long wp_seq_attn(const float* W, int d, uint16_t* out, long cap, float* scale) {
  return give(fdmi::pack_seq_attn(W, d), out, cap, scale);
}
long wp_seq_attn16(const float* W, int d, uint16_t* out, long cap, float* scale) {
  return give(fdmi::pack_seq_attn16(W, d), out, cap, scale);
}
// Wo may be null (no tail stream: *n_tail = 0); scales = first dense | second dense | attention.output.dense
long wp_ffn16(const float* Wi, const float* Wd, const float* Wo, int d, int ff, uint16_t* plain, long cap_plain, uint16_t* tail,
              long cap_tail, long* n_tail, float* scales) {
  const fdmi::Ffn16Images im = fdmi::pack_ffn16(Wi, Wd, Wo, d, ff);
  scales[0] = im.plain.scale;
  scales[1] = im.scale_dn;
  scales[2] = im.tail.scale;
  *n_tail = give(im.tail.data, tail, cap_tail);
  return give(im.plain.data, plain, cap_plain);
}
int wp_permuted_row(int i, int j) { return fdmi::permuted_row(i, j); }
float wp_scale_for(float bound) { return fdmi::scale_for(bound); }
float wp_dense_bound(const float* W, const float* bias, int r0, int r1, int K, float in_l2) {
  return fdmi::dense_bound(W, bias, r0, r1, K, in_l2);
}
void wp_ln_bound(const float* g, const float* b, long d, float extra_each, float* linf_l2) {
  const fdmi::Bound bd = fdmi::ln_bound(g, b, (size_t)d, extra_each);
  linf_l2[0] = bd.linf;
  linf_l2[1] = bd.l2;
}

}  // extern "C"
