// The model's weights: fd_set_weight collects the state_dict on the host, fd_finalize uploads it -- the fp32 tensors as they
// are, and for FD_PREC_F16X3 the byte images and static scales that weight_pack.h computes from them (all the arithmetic is
// there; this file only decides which images a configuration gets and copies them to the device).  Boundary: include/fdmi.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/fdmi.h"
#include "fdmi_kernels.h"
#include "host_common.h"
#include "model.h"
#include "weight_pack.h"

using namespace fdmi;

namespace {

// host bytes to a device buffer that the model owns (free_weights)
int upload_bytes(fd_model* m, void** out, const void* src, size_t bytes) {
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  m->allocs.push_back(p);
  HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
  *out = p;
  return FD_OK;
}
int upload(fd_model* m, float** out, const float* src, size_t n) { return upload_bytes(m, reinterpret_cast<void**>(out), src, n * sizeof(float)); }
int upload_image(fd_model* m, SplitW* dst, const std::vector<uint16_t>& img) { return upload_bytes(m, &dst->p, img.data(), img.size() * 2); }
int upload_image(fd_model* m, SplitW* dst, const Image& im) {
  dst->scale = im.scale;
  return upload_image(m, dst, im.data);
}

// expected shape of a state_dict entry; returns false if the name is not a parameter we consume
bool expected_shape(const fd_config& c, const std::string& name, std::vector<int64_t>* shp, bool* ignored) {
  *ignored = false;
  const int64_t d = c.d_model, F = c.n_features, ff = c.d_ff;
  auto set = [&](std::initializer_list<int64_t> s) { *shp = s; return true; };
  if (name == "time_embed.W" || name == "embeddings.position_ids") { *ignored = true; return true; }
  if (name == "inputs_to_hidden_dim.weight") return set({d, F});
  if (name == "inputs_to_hidden_dim.bias") return set({d});
  if (name == "embeddings.LayerNorm.weight" || name == "embeddings.LayerNorm.bias") return set({d});
  if (name == "embeddings.position_embeddings.weight") return set({c.max_pos, d});
  if (c.decoder == FD_DEC_MLP) {
    if (name == "token_decoder.dense1.weight") return set({d, d});
    if (name == "token_decoder.dense1.bias") return set({d});
    if (name == "token_decoder.layer_norm.weight" || name == "token_decoder.layer_norm.bias") return set({d});
    if (name == "token_decoder.dense2.weight") return set({F, d});
    if (name == "token_decoder.dense2.bias") return set({F});
  } else {
    if (name == "token_decoder.weight") return set({F, d});
    if (name == "token_decoder.bias") return set({F});
  }
  const std::string pre = "encoder.layer.";
  if (name.compare(0, pre.size(), pre) == 0) {
    size_t dot = name.find('.', pre.size());
    if (dot == std::string::npos) return false;
    int li = atoi(name.substr(pre.size(), dot - pre.size()).c_str());
    if (li < 0 || li >= c.n_layers) return false;
    const std::string rest = name.substr(dot + 1);
    for (const char* p : {"attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"}) {
      if (rest == std::string(p) + ".weight") return set({d, d});
      if (rest == std::string(p) + ".bias") return set({d});
    }
    if (rest == "attention.self.distance_embedding.weight") return set({2 * (int64_t)c.max_pos - 1, (int64_t)(c.d_model / c.n_heads)});
    for (const char* p : {"attention.output.LayerNorm", "output.LayerNorm"}) {
      if (rest == std::string(p) + ".weight" || rest == std::string(p) + ".bias") return set({d});
    }
    if (rest == "intermediate.dense.weight") return set({ff, d});
    if (rest == "intermediate.dense.bias") return set({ff});
    if (rest == "output.dense.weight") return set({d, ff});
    if (rest == "output.dense.bias") return set({d});
  }
  return false;
}

const HostTensor* need(fd_model* m, const std::string& name) {
  auto it = m->host.find(name);
  if (it == m->host.end()) {
    fail(FD_E_MISSING, "weight '%s' was never provided (fd_set_weight)", name.c_str());
    return nullptr;
  }
  return &it->second;
}

}  // namespace

void fdmi::free_weights(fd_model* m) {
  for (void* p : m->allocs) (void)hipFree(p);
  m->allocs.clear();
  m->layers.clear();
  m->finalized = false;
}

extern "C" {

int fd_set_weight(fd_model* m, const char* name, const float* host_data, const int64_t* shape, int ndim) {
  if (!m || !name || !host_data || (ndim > 0 && !shape)) return fail(FD_E_INVALID, "null argument");
  std::vector<int64_t> want;
  bool ignored = false;
  if (!expected_shape(m->cfg, name, &want, &ignored)) return fail(FD_E_INVALID, "unexpected state_dict entry '%s'", name);
  if (ignored) return FD_OK;
  std::vector<int64_t> got(shape, shape + ndim);
  if (got != want) {
    std::string a, b;
    for (auto v : got) a += std::to_string(v) + ",";
    for (auto v : want) b += std::to_string(v) + ",";
    return fail(FD_E_INVALID, "'%s': shape [%s] does not match config [%s]", name, a.c_str(), b.c_str());
  }
  size_t n = 1;
  for (auto v : got) n *= (size_t)v;
  HostTensor& t = m->host[name];
  t.shape = got;
  t.data.assign(host_data, host_data + n);
  m->finalized = false;
  return FD_OK;
}

int fd_finalize(fd_model* m, int T, const float* coef, const float* time_table, const uint8_t* is_angle, int precision) {
  if (!m || !coef || !time_table || !is_angle) return fail(FD_E_INVALID, "null argument");
  if (T < 1) return fail(FD_E_INVALID, "T=%d", T);
  if (precision != FD_PREC_F32 && precision != FD_PREC_F16X3) return fail(FD_E_UNSUPPORTED, "precision mode %d", precision);
  if (precision == FD_PREC_F32 && head_dim(m->cfg) != kHeadDim)
    return fail(FD_E_UNSUPPORTED, "head size %d: the exact-fp32 attention kernel is built for head size %d; use FD_PREC_F16X3", head_dim(m->cfg), kHeadDim);
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  drop_workspaces(m);
  free_weights(m);
  const fd_config& c = m->cfg;
  const size_t d = c.d_model, F = c.n_features, ff = c.d_ff;
  // FD_PREC_F16X3 runs on the row-image kernels; the attention-output / FFN-down LayerNorm is fused into the GEMM when a row
  // fits one 384-column workgroup tile (d_model <= 384: every released configuration), else it is its own launch
  const bool img = precision == FD_PREC_F16X3;
  m->img = img;
#define NEED(var, nm)                         \
  const HostTensor* var = need(m, nm);        \
  if (!var) return FD_E_MISSING
#define UP(dst, t) \
  if (int rc_ = upload(m, &(dst), (t)->data.data(), (t)->data.size())) return rc_
#define IMG(dst, image) \
  if (int rc_ = upload_image(m, &(dst), image)) return rc_
  NEED(t_win, "inputs_to_hidden_dim.weight");
  NEED(t_bin, "inputs_to_hidden_dim.bias");
  NEED(t_eg, "embeddings.LayerNorm.weight");
  NEED(t_eb, "embeddings.LayerNorm.bias");
  UP(m->w_in, t_win);
  UP(m->b_in, t_bin);
  UP(m->emb_g, t_eg);
  UP(m->emb_b, t_eb);
  // bound of the hidden state entering layer 0: embeddings LayerNorm + time embedding (|sin|, |cos| <= 1)
  Bound hb = ln_bound(t_eg->data.data(), t_eb->data.data(), d, 1.0f);
  m->pos_emb = nullptr;
  if (c.pos_type == FD_POS_ABSOLUTE) {
    NEED(t_pe, "embeddings.position_embeddings.weight");
    UP(m->pos_emb, t_pe);
  }
  m->layers.resize(c.n_layers);
  for (int li = 0; li < c.n_layers; ++li) {
    const std::string p = "encoder.layer." + std::to_string(li) + ".";
    LayerDev& lw = m->layers[li];
    NEED(wq, p + "attention.self.query.weight");
    NEED(wk, p + "attention.self.key.weight");
    NEED(wv, p + "attention.self.value.weight");
    NEED(bq, p + "attention.self.query.bias");
    NEED(bk, p + "attention.self.key.bias");
    NEED(bv, p + "attention.self.value.bias");
    std::vector<float> wqkv, bqkv;  // rows: [query | key | value]  => one N = 3d GEMM
    wqkv.reserve(3 * d * d);
    for (const HostTensor* t : {wq, wk, wv}) wqkv.insert(wqkv.end(), t->data.begin(), t->data.end());
    for (const HostTensor* t : {bq, bk, bv}) bqkv.insert(bqkv.end(), t->data.begin(), t->data.end());
    if (int rc = upload(m, &lw.wqkv, wqkv.data(), wqkv.size())) return rc;
    if (int rc = upload(m, &lw.bqkv, bqkv.data(), bqkv.size())) return rc;
    if (img) {
      IMG(lw.wqk_i, pack_weight_tiles(wqkv.data(), 2 * (int)d, (int)d));
      IMG(lw.wv_i, pack_weight_tiles(wqkv.data() + 2 * d * d, (int)d, (int)d));
      if (sub_heads(c) % 6 == 0) IMG(lw.wqkv_i, pack_weight_tiles(wqkv.data(), 3 * (int)d, (int)d));
      if (c.pos_type == FD_POS_RELATIVE_KEY && seq_attn_supported((int)d, c.n_heads, c.max_pos < 128 ? c.max_pos : 128, c.max_pos))
        IMG(lw.wsa_i, pack_seq_attn(wqkv.data(), (int)d));
      if (c.pos_type == FD_POS_RELATIVE_KEY && seq_attn16_supported((int)d, c.n_heads, c.max_pos < 128 ? c.max_pos : 128, c.max_pos))
        IMG(lw.wsa16_i, pack_seq_attn16(wqkv.data(), (int)d));
      lw.bqk = lw.bqkv;
      lw.bv = lw.bqkv + 2 * d;
      lw.s_h = scale_for(hb.linf);
      lw.s_q = scale_for(dense_bound(wqkv.data(), bqkv.data(), 0, (int)d, (int)d, hb.l2));
      lw.s_k = scale_for(dense_bound(wqkv.data(), bqkv.data(), (int)d, 2 * (int)d, (int)d, hb.l2));
      lw.s_v = scale_for(dense_bound(wqkv.data(), bqkv.data(), 2 * (int)d, 3 * (int)d, (int)d, hb.l2));  // also bounds ctx
    }
    lw.demb = nullptr;
    if (c.pos_type != FD_POS_ABSOLUTE) {  // relative_key and relative_key_query
      NEED(de, p + "attention.self.distance_embedding.weight");
      UP(lw.demb, de);
      if (precision == FD_PREC_F16X3) IMG(lw.demb_s, pack_split_weight(de->data.data(), 2 * c.max_pos - 1, head_dim(c)));
    }
    NEED(wo, p + "attention.output.dense.weight");
    NEED(bo, p + "attention.output.dense.bias");
    NEED(g1, p + "attention.output.LayerNorm.weight");
    NEED(b1, p + "attention.output.LayerNorm.bias");
    NEED(wi, p + "intermediate.dense.weight");
    NEED(bi, p + "intermediate.dense.bias");
    NEED(wd, p + "output.dense.weight");
    NEED(bd, p + "output.dense.bias");
    NEED(g2, p + "output.LayerNorm.weight");
    NEED(b2, p + "output.LayerNorm.bias");
    UP(lw.wo, wo); UP(lw.bo, bo); UP(lw.ln1g, g1); UP(lw.ln1b, b1);
    UP(lw.wi, wi); UP(lw.bi, bi); UP(lw.wd, wd); UP(lw.bd, bd); UP(lw.ln2g, g2); UP(lw.ln2b, b2);
    if (img) {
      IMG(lw.wo_i, pack_weight_tiles(wo->data.data(), (int)d, (int)d));
      IMG(lw.wi_i, pack_weight_tiles(wi->data.data(), (int)ff, (int)d));
      IMG(lw.wd_i, pack_weight_tiles(wd->data.data(), (int)d, (int)ff));
      if (ffn16_supported((int)d, (int)ff)) {
        const Ffn16Images f = pack_ffn16(wi->data.data(), wd->data.data(), wo->data.data(), (int)d, (int)ff);
        IMG(lw.wff_i, f.plain);
        lw.wff_scale_dn = f.scale_dn;
        IMG(lw.wtail_i, f.tail);
      }
      const Bound ab = ln_bound(g1->data.data(), b1->data.data(), d);
      lw.s_a = scale_for(ab.linf);
      lw.s_g = scale_for(dense_bound(wi->data.data(), bi->data.data(), 0, (int)ff, (int)d, ab.l2));  // |gelu(u)| <= |u|
      hb = ln_bound(g2->data.data(), b2->data.data(), d);  // hidden state entering the next layer
    }
  }
  m->s_hfinal = scale_for(hb.linf);
  if (c.decoder == FD_DEC_MLP) {
    NEED(w1, "token_decoder.dense1.weight");
    NEED(b1, "token_decoder.dense1.bias");
    NEED(g, "token_decoder.layer_norm.weight");
    NEED(b, "token_decoder.layer_norm.bias");
    NEED(w2, "token_decoder.dense2.weight");
    NEED(b2, "token_decoder.dense2.bias");
    UP(m->hd_w1, w1); UP(m->hd_b1, b1); UP(m->hd_g, g); UP(m->hd_b, b); UP(m->hd_w2, w2); UP(m->hd_b2, b2);
    if (img) {
      IMG(m->hd_w1_i, pack_weight_tiles(w1->data.data(), (int)d, (int)d));
      m->s_hg = scale_for(dense_bound(w1->data.data(), b1->data.data(), 0, (int)d, (int)d, hb.l2));
    }
  } else {
    NEED(w2, "token_decoder.weight");
    NEED(b2, "token_decoder.bias");
    UP(m->hd_w2, w2); UP(m->hd_b2, b2);
  }
#undef NEED
#undef UP
#undef IMG
  if (int rc = upload(m, &m->coef, coef, (size_t)4 * T)) return rc;
  if (int rc = upload(m, &m->time_table, time_table, (size_t)T * d)) return rc;
  m->angle_mask = 0;
  for (size_t f = 0; f < F; ++f)
    if (is_angle[f]) m->angle_mask |= 1u << f;
  m->T = T;
  m->precision = precision;
  m->finalized = true;
  return FD_OK;
}

}  // extern "C"
