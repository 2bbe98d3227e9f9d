// C-ABI entry points of the structure kernels (nerf.hip, internal_coords.hip, tm_score.hip, psea.hip, dssp.hip, tm_align.hip, tm_align_starts.hip, clash_lddt.hip), of
// the loss arithmetic on its own (loss.hip, loss_variants.hip), of the angle histograms (angle_stats.hip) of the steering kernels on their own (steer.hip), of the NeRF derivative, the restraints and the guide step (nerf_vjp.hip), of the torsion-space relaxer (nerf_scan.hip, relax.hip) of the scaffold-guide step (guide_scaffold.hip) of the superposition restraints (template_fit.hip) and of the cyclic-symmetry statements (symmetry.hip).  None of them sees a model: each takes a device_id, checks its arguments on the host, and makes one synchronous
// round trip (host_common.h).  Boundary: include/fdmi.h.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "fdmi_kernels.h"
#include "host_common.h"
#include "symmetry_host.h"

using namespace fdmi;

// the six uploads of a batch's restraints (check_restraints has passed); an empty list uploads one entry per array, never read
namespace {
struct RestraintInputs {
  std::pair<const void*, size_t> offsets, i, j, d0, tol, w;
};
RestraintInputs restraint_inputs(const RestraintLists& r) {
  static const int32_t no_atom = 0;
  static const double no_value = 0.0;
  const size_t R = r.count();
  const auto ints = [&](const int32_t* p) { return std::pair<const void*, size_t>(R ? p : &no_atom, (R ? R : 1) * 4); };
  const auto doubles = [&](const double* p) { return std::pair<const void*, size_t>(R ? p : &no_value, (R ? R : 1) * 8); };
  return {{r.offsets, ((size_t)r.n_chains + 1) * 4}, ints(r.i), ints(r.j), doubles(r.d0), doubles(r.tol), doubles(r.w)};
}
// the four uploads of a batch's templates (check_template has passed); none: B + 1 zero offsets; no entry: one per array, never read
struct TemplateInputs {
  std::vector<int32_t> no_offsets;
  std::pair<const void*, size_t> offsets, atom, xyz, w;
};
TemplateInputs template_inputs(const TemplateLists& t) {
  static const int32_t no_atom = 0;
  static const double no_value[3] = {0.0, 0.0, 0.0};
  TemplateInputs r;
  const size_t n = t.count(), nb = (size_t)t.n_chains + 1;
  if (t.none()) r.no_offsets.assign(nb, 0);
  r.offsets = {t.none() ? r.no_offsets.data() : t.offsets, nb * 4};
  r.atom = {n ? (const void*)t.atom : &no_atom, (n ? n : 1) * 4};
  r.xyz = {n ? (const void*)t.xyz : no_value, (n ? n : 1) * 24};
  r.w = {n ? (const void*)t.w : no_value, (n ? n : 1) * 8};
  return r;
}
}  // namespace

extern "C" {

int fd_nerf(int device_id, const float* feats, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
            int center, double* coords_out) {
  if (!feats || !lens || !feat_idx || !coords_out || B < 1 || L < 1 || F < 3) return fail(FD_E_INVALID, "bad argument");
  for (int i = 0; i < 9; ++i)
    if (feat_idx[i] >= F || (i < 3 && feat_idx[i] < 0)) return fail(FD_E_INVALID, "feat_idx[%d]=%d (F=%d)", i, feat_idx[i], F);
  if (int rc = check_lens(lens, B, L)) return rc;
  const NerfFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5], feat_idx[6], feat_idx[7], feat_idx[8]};
  return device_roundtrip(device_id, {{feats, (size_t)B * L * F * 4}, {lens, (size_t)B * 4}},
                          {{coords_out, (size_t)B * 3 * L * 3 * 8}},
                          [&](const RoundtripBufs& d) { launch_nerf(d.in(0), d.in(1), B, L, F, fx, center, d.out(0), nullptr); });
}

// fd_nerf_vjp (feats == nullptr: every sign +1) and fd_nerf_vjp_feats
static int nerf_vjp_run(int device_id, const double* coords, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                        int centered, const double* dcoords, const float* feats, bool with_feats, double* dfeats_out) {
  if (!coords || !lens || !feat_idx || !dcoords || !dfeats_out || (with_feats && !feats)) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_guide_shape(lens, B, L, F, feat_idx)) return rc;
  if (int rc = check_chain_doubles("coords", coords, lens, B, L)) return rc;
  if (int rc = check_chain_doubles("dcoords", dcoords, lens, B, L)) return rc;
  if (with_feats)
    if (int rc = check_rows_finite("feats", feats, lens, B, L, F)) return rc;
  const NerfFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5], feat_idx[6], feat_idx[7], feat_idx[8]};
  const size_t na = (size_t)B * 3 * L * 3, n = (size_t)B * L * F;
  std::vector<double> grad_host(n);  // the rows at or beyond a length are not the kernel's: dfeats_out keeps what it held there
  const int rc = device_roundtrip(device_id, {{coords, na * 8}, {dcoords, na * 8}, {lens, (size_t)B * 4}, {with_feats ? (const void*)feats : (const void*)coords, with_feats ? n * 4 : 4}},
                                  {{grad_host.data(), n * 8}}, [&](const RoundtripBufs& d) {
                                    const float* rows = d.in(3);
                                    launch_nerf_vjp(d.in(0), d.in(2), B, L, F, fx, centered, d.in(1), with_feats ? rows : nullptr, d.out(0), nullptr);
                                  });
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    memcpy(dfeats_out + (size_t)b * L * F, grad_host.data() + (size_t)b * L * F, (size_t)lens[b] * F * 8);
  return FD_OK;
}

int fd_nerf_vjp(int device_id, const double* coords, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx, int centered,
                const double* dcoords, double* dfeats_out) {
  return nerf_vjp_run(device_id, coords, lens, B, L, F, feat_idx, centered, dcoords, nullptr, false, dfeats_out);
}

int fd_nerf_vjp_feats(int device_id, const double* coords, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                      int centered, const double* dcoords, const float* feats, double* dfeats_out) {
  return nerf_vjp_run(device_id, coords, lens, B, L, F, feat_idx, centered, dcoords, feats, true, dfeats_out);
}

int fd_restraint_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* rst_offsets,
                        const int32_t* rst_i, const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                        double* energy_out, double* max_violation_out, double* dcoords_out) {
  if (!coords || !lens || !energy_out || !max_violation_out) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if ((long long)B * L * 9 > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * 9 = %lld coordinates, at most 2^31 - 1", (long long)B * L * 9);
  if (int rc = check_lens(lens, B, L < kGuideMaxLen ? L : kGuideMaxLen)) return rc;
  const RestraintLists rl{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w};
  if (int rc = check_restraints(rl, lens)) return rc;
  if (int rc = check_chain_doubles("coords", coords, lens, B, L)) return rc;
  const RestraintInputs ri = restraint_inputs(rl);
  const size_t na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  return device_roundtrip(device_id, {{coords, na * 8}, {lens, nb * 4}, ri.offsets, ri.i, ri.j, ri.d0, ri.tol, ri.w},
                          {{energy_out, nb * 8}, {max_violation_out, nb * 8}, {dcoords_out, dcoords_out ? na * 8 : 8}},
                          [&](const RoundtripBufs& d) {
                            const Restraints rs{d.in(2), d.in(3), d.in(4), d.in(5), d.in(6), d.in(7)};
                            double* grad = d.out(2);
                            launch_restraint_energy(d.in(0), d.in(1), B, L, rs, d.out(0), d.out(1), dcoords_out ? grad : nullptr, nullptr);
                          });
}

int fd_template_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* tpl_offsets,
                       const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w, double* energy_out, double* rmsd_out,
                       double* transform_out, double* dcoords_out) {
  if (!coords || !lens || !energy_out || !rmsd_out) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if ((long long)B * L * 9 > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * 9 = %lld coordinates, at most 2^31 - 1", (long long)B * L * 9);
  if (int rc = check_lens(lens, B, L < kGuideMaxLen ? L : kGuideMaxLen)) return rc;
  const TemplateLists tl{B, tpl_offsets, tpl_atom, tpl_xyz, tpl_w};
  if (int rc = check_template(tl, lens)) return rc;
  if (int rc = check_chain_doubles("coords", coords, lens, B, L)) return rc;
  const TemplateInputs ti = template_inputs(tl);
  const size_t na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  return device_roundtrip(device_id, {{coords, na * 8}, ti.offsets, ti.atom, ti.xyz, ti.w},
                          {{energy_out, nb * 8}, {rmsd_out, nb * 8}, {transform_out, transform_out ? nb * 96 : 8}, {dcoords_out, dcoords_out ? na * 8 : 8}},
                          [&](const RoundtripBufs& d) -> hipError_t {
                            const TemplateFit tf{d.in(1), d.in(2), d.in(3), d.in(4)};
                            double *T = d.out(2), *grad = d.out(3);
                            if (dcoords_out)  // (the launch adds: the atoms it does not name stay 0)
                              if (hipError_t e = hipMemsetAsync(grad, 0, na * 8, nullptr)) return e;
                            launch_template_energy(d.in(0), B, L, tf, d.out(0), d.out(1), transform_out ? T : nullptr, dcoords_out ? grad : nullptr, nullptr);
                            return hipSuccess;
                          });
}

int fd_guide_step(int device_id, const float* x, const float* x0, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                  const float* offset, const uint8_t* is_angle, const int32_t* rst_offsets, const int32_t* rst_i,
                  const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float c, double max_norm,
                  float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                  double* gnorm_out) {
  if (!x || !x0 || !lens || !feat_idx || !is_angle || !x_out || !energy_out || !gnorm_out) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_guide_shape(lens, B, L, F, feat_idx)) return rc;
  const RestraintLists rl{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w};
  if (int rc = check_restraints(rl, lens)) return rc;
  if (!std::isfinite(c)) return fail(FD_E_INVALID, "c = %g is not finite", (double)c);
  if (!std::isfinite(s)) return fail(FD_E_INVALID, "s = %g is not finite", (double)s);
  if (int rc = check_guide_scalars(max_norm, offset, F)) return rc;
  if (int rc = check_rows_finite("x", x, lens, B, L, F)) return rc;
  if (int rc = check_rows_finite("x0", x0, lens, B, L, F)) return rc;
  const NerfFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5], feat_idx[6], feat_idx[7], feat_idx[8]};
  SteerOffset off{};
  off.has_offset = offset ? 1 : 0;
  unsigned angle_mask = 0;
  for (int f = 0; f < F; ++f) {
    if (offset) off.offset[f] = offset[f];
    if (is_angle[f]) angle_mask |= 1u << f;
  }
  const RestraintInputs ri = restraint_inputs(rl);
  const size_t n = (size_t)B * L * F, na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  const bool draws = s != 0.f && z;  // (the slab is read only then)
  std::vector<float> state_host(n);  // the rows at or beyond a length are not the kernels': x_out keeps what it held there
  const int rc = device_roundtrip(
      device_id, {{x, n * 4}, {x0, n * 4}, {lens, nb * 4}, {draws ? z : x, draws ? n * 4 : 4}, ri.offsets, ri.i, ri.j, ri.d0, ri.tol, ri.w},
      {{state_host.data(), n * 4}, {nullptr, n * 4}, {nullptr, na * 8}, {nullptr, na * 8}, {nullptr, n * 8}, {energy_out, nb * 8},
       {nullptr, nb * 8}, {gnorm_out, nb * 8}},
      [&](const RoundtripBufs& d) -> hipError_t {
        float *state = d.out(0), *ang = d.out(1);
        double *coords = d.out(2), *gc = d.out(3), *G = d.out(4);
        const float *x_dev = d.in(0), *z_dev = d.in(3);
        const int* lens_dev = d.in(2);
        const Restraints rs{d.in(4), d.in(5), d.in(6), d.in(7), d.in(8), d.in(9)};
        if (hipError_t e = hipMemcpyAsync(state, x_dev, n * 4, hipMemcpyDeviceToDevice, nullptr)) return e;
        launch_steer_shift(d.in(1), lens_dev, B, L, F, off, angle_mask, ang, nullptr);
        launch_nerf(ang, lens_dev, B, L, F, fx, 0, coords, nullptr);
        launch_restraint_energy(coords, lens_dev, B, L, rs, d.out(5), d.out(6), gc, nullptr);
        launch_nerf_vjp(coords, lens_dev, B, L, F, fx, 0, gc, ang, G, nullptr);
        launch_guide_update(state, G, lens_dev, B, L, F, angle_mask, c, max_norm, s, draws ? z_dev : nullptr, seed, t, seq_offset,
                            d.out(7), nullptr);
        return hipSuccess;
      });
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    memcpy(x_out + (size_t)b * L * F, state_host.data() + (size_t)b * L * F, (size_t)lens[b] * F * 4);
  return FD_OK;
}

}  // extern "C"

// fd_scaffold_guide_step_sym's own arguments; order == nullptr: no symmetry, and nothing else is looked at
namespace {
struct SymStepArgs {
  const int32_t* order;
  const double *pose_in, *placed_in;
  const fd_symmetry_params* params;
  double* step_io;
  double* energy_out;
  int32_t* contacts_out;
  double *pose_out, *placed_out;
};
}  // namespace

// fd_scaffold_guide_step (energy_out [B][2], tpl_rmsd_out == nullptr, no template), fd_scaffold_guide_step_tpl ([B][3]) and
// fd_scaffold_guide_step_sym (sym != nullptr)
static int scaffold_guide_step_run(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                                   const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                                   const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                                   const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                                   const TemplateLists& tl, int n_energies, float c, float s, const float* z, uint64_t seed, int t,
                                   int64_t seq_offset, float* x_out, double* energy_out, double* max_violation_out, double* gnorm_out,
                                   double* dfeats_out, double* tpl_rmsd_out, const SymStepArgs* sym = nullptr) {
  if (!x || !x0 || !lens || !is_angle || !params || !x_out || !energy_out || !max_violation_out || !gnorm_out ||
      (n_energies == 3 && !tpl_rmsd_out))
    return fail(FD_E_INVALID, "null argument");
  if (!known) return fail(FD_E_INVALID, "known is null");
  if (!fixed) return fail(FD_E_INVALID, "fixed is null");
  if (int rc = check_guide_shape(lens, B, L, F, params->feat_idx)) return rc;
  const RestraintLists rl{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w};
  if (int rc = check_restraints(rl, lens)) return rc;
  if (int rc = check_template(tl, lens)) return rc;
  if (!std::isfinite(c)) return fail(FD_E_INVALID, "c = %g is not finite", (double)c);
  if (!std::isfinite(s)) return fail(FD_E_INVALID, "s = %g is not finite", (double)s);
  if (int rc = check_scaffold_guide(*params, known, fixed, lens, B, L, F)) return rc;
  if (int rc = check_rows_finite("x", x, lens, B, L, F)) return rc;
  bool symmetric = false;  // a chain has an order above 1: only then do the symmetry launches run
  if (sym && sym->order) {
    if (!sym->pose_in || !sym->params || !sym->energy_out || !sym->contacts_out || !sym->pose_out || !sym->placed_out)
      return fail(FD_E_INVALID, "null argument: the symmetry arrays");
    if (int rc = check_symmetry(*sym->params, sym->order, sym->pose_in, B)) return rc;
    for (int b = 0; sym->step_io && b < B; ++b)
      if (!(sym->step_io[b] > 0.0) || !std::isfinite(sym->step_io[b]))
        return fail(FD_E_INVALID, "sym_step_io[%d]=%g must be > 0 and finite", b, sym->step_io[b]);
    if (sym->placed_in)
      if (int rc = check_chain_doubles("sym_placed_in", sym->placed_in, lens, B, L)) return rc;
    for (int b = 0; b < B; ++b) symmetric |= sym->order[b] >= 2;
  }
  for (int b = 0; b < B; ++b)  // (x0 is not read where fixed)
    for (size_t o = (size_t)b * L * F; o < ((size_t)b * L + lens[b]) * F; ++o)
      if (!fixed[o] && !std::isfinite(x0[o]))
        return fail(FD_E_INVALID, "x0 is not finite at a free element: sequence %d, position %d", b, (int)(o / F - (size_t)b * L));
  const fd_scaffold_guide_params& p = *params;
  const NerfFeatures fx{p.feat_idx[0], p.feat_idx[1], p.feat_idx[2], p.feat_idx[3], p.feat_idx[4], p.feat_idx[5], p.feat_idx[6], p.feat_idx[7], p.feat_idx[8]};
  SteerOffset off{};
  off.has_offset = p.has_offset ? 1 : 0;
  unsigned angle_mask = 0;
  for (int f = 0; f < F; ++f) {
    if (p.has_offset) off.offset[f] = p.offset[f];
    if (is_angle[f]) angle_mask |= 1u << f;
  }
  const SoftClash clash{p.clash_alpha, p.clash_margin, p.w_clash};
  const RestraintInputs ri = restraint_inputs(rl);
  const size_t n = (size_t)B * L * F, na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  const bool draws = s != 0.f && z;  // (the slab is read only then)
  HIP_TRY(hipSetDevice(device_id));
  DeviceBufs bufs;
  float* state;
  const float *x0_dev, *known_dev, *z_dev = nullptr;
  const unsigned char* fixed_dev;
  const int* lens_dev;
  Restraints rs{};
  ScaffoldWork wk{};
  double *G, *gnorm;
  HIP_TRY(bufs.upload(x, n * 4, &state));
  HIP_TRY(bufs.upload(x0, n * 4, &x0_dev));
  HIP_TRY(bufs.upload(known, n * 4, &known_dev));
  HIP_TRY(bufs.upload(fixed, n, &fixed_dev));
  HIP_TRY(bufs.upload(lens, nb * 4, &lens_dev));
  if (draws) HIP_TRY(bufs.upload(z, n * 4, &z_dev));
  HIP_TRY(bufs.upload(ri.offsets.first, ri.offsets.second, &rs.offsets));
  HIP_TRY(bufs.upload(ri.i.first, ri.i.second, &rs.i));
  HIP_TRY(bufs.upload(ri.j.first, ri.j.second, &rs.j));
  HIP_TRY(bufs.upload(ri.d0.first, ri.d0.second, &rs.d0));
  HIP_TRY(bufs.upload(ri.tol.first, ri.tol.second, &rs.tol));
  HIP_TRY(bufs.upload(ri.w.first, ri.w.second, &rs.w));
  HIP_TRY(bufs.alloc(n * 4, &wk.ang));
  HIP_TRY(bufs.alloc(na * 8, &wk.coords));
  HIP_TRY(bufs.alloc(na * 8, &wk.gc));
  HIP_TRY(bufs.alloc(nb * 8, &wk.e_rst));
  HIP_TRY(bufs.alloc(nb * 8, &wk.max_violation));
  HIP_TRY(bufs.zeros(nb * 8, &wk.e_clash));  // (stays 0 where there is no clash term)
  HIP_TRY(bufs.zeros(nb * 8, &wk.e_tpl));    // (and these where no chain has a template entry)
  HIP_TRY(bufs.zeros(nb * 8, &wk.rmsd_tpl));
  HIP_TRY(bufs.alloc(n * 8, &G));
  HIP_TRY(bufs.alloc(nb * 8, &gnorm));
  TemplateFit tf{};
  const bool fit = tl.count() > 0;
  if (fit) {
    HIP_TRY(bufs.upload(tl.offsets, (nb + 1) * 4, &tf.offsets));
    HIP_TRY(bufs.upload(tl.atom, tl.count() * 4, &tf.atom));
    HIP_TRY(bufs.upload(tl.xyz, tl.count() * 24, &tf.xyz));
    HIP_TRY(bufs.upload(tl.w, tl.count() * 8, &tf.w));
  }
  SymGuide sg{};
  std::vector<SymState> sym_host(symmetric ? nb : 0);
  if (symmetric) {
    if (int rc = stage_symmetry_guide(&bufs, sym->order, sym->pose_in, sym->step_io, *sym->params, lens, lens_dev, wk.coords, B, L,
                                      sym->placed_in, false, &sg))
      return rc;
    HIP_TRY(bufs.zeros(na * 8, &sg.placed));
  }
  launch_scaffold_energy(x0_dev, known_dev, fixed_dev, lens_dev, B, L, F, off, angle_mask, fx, rs, clash, fit ? &tf : nullptr, wk, G, nullptr,
                         symmetric ? &sg : nullptr);
  launch_scaffold_update(state, G, fixed_dev, lens_dev, B, L, F, angle_mask, c, p.max_norm, s, z_dev, seed, t, seq_offset, gnorm, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<float> state_host(n);
  std::vector<double> grad_host(dfeats_out ? n : 0), e_rst(nb), e_clash(nb), maxv(nb), norm(nb), e_tpl(nb), rmsd_tpl(nb);
  HIP_TRY(hipMemcpy(e_tpl.data(), wk.e_tpl, nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rmsd_tpl.data(), wk.rmsd_tpl, nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(state_host.data(), state, n * 4, hipMemcpyDeviceToHost));
  if (dfeats_out) HIP_TRY(hipMemcpy(grad_host.data(), G, n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(e_rst.data(), wk.e_rst, nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(e_clash.data(), wk.e_clash, nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(maxv.data(), wk.max_violation, nb * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(norm.data(), gnorm, nb * 8, hipMemcpyDeviceToHost));
  std::vector<double> sym_e(symmetric ? nb * 3 : 0), sym_placed(symmetric ? na : 0);
  std::vector<int32_t> sym_c(symmetric ? nb : 0);
  if (symmetric) {
    HIP_TRY(hipMemcpy(sym_host.data(), sg.dock.state, nb * sizeof(SymState), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sym_e.data(), sg.energy, nb * 24, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sym_c.data(), sg.contacts, nb * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sym_placed.data(), sg.placed, na * 8, hipMemcpyDeviceToHost));
  }
  // every download has succeeded: only now are the outputs written (the rows at or beyond a length keep what they held)
  for (int b = 0; sym && sym->order && b < B; ++b) {
    for (int k = 0; k < 3; ++k) sym->energy_out[3 * b + k] = symmetric ? sym_e[3 * (size_t)b + k] : 0.0;
    sym->contacts_out[b] = symmetric ? sym_c[b] : 0;
    memcpy(sym->pose_out + 12 * (size_t)b, symmetric ? sym_host[b].pose : sym->pose_in + 12 * (size_t)b, 96);
    if (symmetric) {
      memcpy(sym->placed_out + (size_t)b * 3 * L * 3, sym_placed.data() + (size_t)b * 3 * L * 3, (size_t)lens[b] * 72);
      if (sym->step_io) sym->step_io[b] = sym_host[b].h;
    }
  }
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * L * F, rows = (size_t)lens[b] * F;
    memcpy(x_out + o, state_host.data() + o, rows * 4);
    if (dfeats_out) memcpy(dfeats_out + o, grad_host.data() + o, rows * 8);
    energy_out[n_energies * b] = e_rst[b];
    energy_out[n_energies * b + 1] = e_clash[b];
    if (n_energies == 3) {
      energy_out[3 * b + 2] = e_tpl[b];
      tpl_rmsd_out[b] = rmsd_tpl[b];
    }
    max_violation_out[b] = maxv[b];
    gnorm_out[b] = norm[b];
  }
  return FD_OK;
}

extern "C" {

int fd_scaffold_guide_step(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                           const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                           const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                           const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, float c, float s,
                           const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                           double* max_violation_out, double* gnorm_out, double* dfeats_out) {
  return scaffold_guide_step_run(device_id, x, x0, known, fixed, lens, B, L, F, is_angle, params, rst_offsets, rst_i, rst_j, rst_d0, rst_tol,
                                 rst_w, TemplateLists{B, nullptr, nullptr, nullptr, nullptr}, 2, c, s, z, seed, t, seq_offset, x_out,
                                 energy_out, max_violation_out, gnorm_out, dfeats_out, nullptr);
}

int fd_scaffold_guide_step_tpl(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                               const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                               const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                               const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                               const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w, float c,
                               float s, const float* z, uint64_t seed, int t, int64_t seq_offset, float* x_out, double* energy_out,
                               double* max_violation_out, double* gnorm_out, double* dfeats_out, double* tpl_rmsd_out) {
  return scaffold_guide_step_run(device_id, x, x0, known, fixed, lens, B, L, F, is_angle, params, rst_offsets, rst_i, rst_j, rst_d0, rst_tol,
                                 rst_w, TemplateLists{B, tpl_offsets, tpl_atom, tpl_xyz, tpl_w}, 3, c, s, z, seed, t, seq_offset, x_out,
                                 energy_out, max_violation_out, gnorm_out, dfeats_out, tpl_rmsd_out);
}

int fd_scaffold_guide_step_sym(int device_id, const float* x, const float* x0, const float* known, const uint8_t* fixed,
                               const int32_t* lens, int B, int L, int F, const uint8_t* is_angle,
                               const fd_scaffold_guide_params* params, const int32_t* rst_offsets, const int32_t* rst_i,
                               const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w,
                               const int32_t* tpl_offsets, const int32_t* tpl_atom, const double* tpl_xyz, const double* tpl_w,
                               const int32_t* sym_order, const double* sym_pose_in, const double* sym_placed_in,
                               const fd_symmetry_params* sym_params, double* sym_step_io, float c, float s, const float* z, uint64_t seed,
                               int t, int64_t seq_offset, float* x_out, double* energy_out, double* max_violation_out, double* gnorm_out,
                               double* dfeats_out, double* tpl_rmsd_out, double* sym_energy_out, int32_t* sym_contacts_out,
                               double* sym_pose_out, double* sym_placed_out) {
  const SymStepArgs sym{sym_order, sym_pose_in, sym_placed_in, sym_params, sym_step_io, sym_energy_out, sym_contacts_out, sym_pose_out, sym_placed_out};
  return scaffold_guide_step_run(device_id, x, x0, known, fixed, lens, B, L, F, is_angle, params, rst_offsets, rst_i, rst_j, rst_d0, rst_tol,
                                 rst_w, TemplateLists{B, tpl_offsets, tpl_atom, tpl_xyz, tpl_w}, 3, c, s, z, seed, t, seq_offset, x_out,
                                 energy_out, max_violation_out, gnorm_out, dfeats_out, tpl_rmsd_out, &sym);
}

int fd_nerf_scan(int device_id, const float* feats, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx, int center,
                 double* coords_out) {
  if (!feats || !lens || !feat_idx || !coords_out) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1 || F < 3) return fail(FD_E_INVALID, "B=%d L=%d F=%d: B, L >= 1 and F >= 3", B, L, F);
  if ((long long)B * L * 9 > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * 9 = %lld coordinates, at most 2^31 - 1", (long long)B * L * 9);
  for (int i = 0; i < 9; ++i)
    if (feat_idx[i] >= F || (i < 3 && feat_idx[i] < 0)) return fail(FD_E_INVALID, "feat_idx[%d]=%d (F=%d)", i, feat_idx[i], F);
  if (int rc = check_lens(lens, B, L < kGuideMaxLen ? L : kGuideMaxLen)) return rc;
  const NerfFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5], feat_idx[6], feat_idx[7], feat_idx[8]};
  return device_roundtrip(device_id, {{feats, (size_t)B * L * F * 4}, {lens, (size_t)B * 4}}, {{coords_out, (size_t)B * 3 * L * 3 * 8}},
                          [&](const RoundtripBufs& d) { launch_nerf_scan(d.in(0), d.in(1), B, L, F, fx, center, d.out(0), nullptr); });
}

// fd_relax_energy (n_iter == 0, descent == false) and fd_relax: the checks, the uploads, 1 + n_iter evaluations, the downloads
static int relax_run(int device_id, const float* feats, const float* anchor, const int32_t* lens, int B, int L, int F,
                     const fd_relax_params* params, const uint8_t* fixed, const RestraintLists& rl, int n_iter, double* step_io,
                     float* feats_out, double* energy_out, double* gnorm_out, double* dfeats_out, double* trace_out,
                     int32_t* accepted_out) {
  if (!feats || !lens || !params || !energy_out) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_guide_shape(lens, B, L, F, params->feat_idx)) return rc;
  if (int rc = check_restraints(rl, lens)) return rc;
  const fd_relax_params& p = *params;
  unsigned angle_mask = 0, move_mask = 0;
  for (int f = 0; f < F; ++f) {
    if (p.is_angle[f]) angle_mask |= 1u << f;
    if (!p.move[f]) continue;
    move_mask |= 1u << f;
    bool named = false;
    for (int i = 0; i < 9; ++i) named |= p.feat_idx[i] == f;
    if (!named) return fail(FD_E_INVALID, "move[%d] is set, but column %d is no NeRF feature of feat_idx", f, f);
  }
  const struct { const char* name; double v; } weights[] = {{"clash_alpha", p.clash_alpha}, {"clash_margin", p.clash_margin},
                                                            {"w_clash", p.w_clash}, {"w_tether", p.w_tether}};
  for (const auto& w : weights)
    if (!(w.v >= 0.0) || !std::isfinite(w.v)) return fail(FD_E_INVALID, "%s=%g must be >= 0 and finite", w.name, w.v);
  if (!(p.step0 > 0.0) || !std::isfinite(p.step0)) return fail(FD_E_INVALID, "step0=%g must be > 0 and finite", p.step0);
  if (!(p.grow >= 1.0) || !std::isfinite(p.grow)) return fail(FD_E_INVALID, "grow=%g must be >= 1 and finite", p.grow);
  if (!(p.shrink > 0.0 && p.shrink < 1.0)) return fail(FD_E_INVALID, "shrink=%g outside (0, 1)", p.shrink);
  if (!(p.max_step > 0.0) || !std::isfinite(p.max_step)) return fail(FD_E_INVALID, "max_step=%g must be > 0 and finite", p.max_step);
  if (n_iter < 0) return fail(FD_E_INVALID, "n_iter=%d must be >= 0", n_iter);
  if ((long long)(n_iter + 1LL) * B > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "(n_iter + 1) * B = %lld trace entries, at most 2^31 - 1", (n_iter + 1LL) * B);
  for (int b = 0; step_io && b < B; ++b)
    if (!(step_io[b] > 0.0) || !std::isfinite(step_io[b])) return fail(FD_E_INVALID, "step_io[%d]=%g must be > 0 and finite", b, step_io[b]);
  if (int rc = check_rows_finite("feats", feats, lens, B, L, F)) return rc;
  if (anchor)
    if (int rc = check_rows_finite("anchor", anchor, lens, B, L, F)) return rc;

  const NerfFeatures fx{p.feat_idx[0], p.feat_idx[1], p.feat_idx[2], p.feat_idx[3], p.feat_idx[4], p.feat_idx[5], p.feat_idx[6], p.feat_idx[7], p.feat_idx[8]};
  const RestraintInputs ri = restraint_inputs(rl);
  const size_t n = (size_t)B * L * F, na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  std::vector<RelaxState> state_host(nb);
  for (size_t b = 0; b < nb; ++b) {
    state_host[b] = RelaxState{};
    state_host[b].h = step_io ? step_io[b] : p.step0;
  }
  HIP_TRY(hipSetDevice(device_id));
  DeviceBufs bufs;
  RelaxStep a{};
  int* lens_dev;
  int *rst_offsets, *rst_i, *rst_j;
  double *rst_d0, *rst_tol, *rst_w, *coords, *gc, *e_clash, *e_rst, *max_violation;
  HIP_TRY(bufs.upload(feats, n * 4, &a.xt));  // the first trial is the input
  HIP_TRY(bufs.upload(anchor ? anchor : feats, n * 4, &a.anchor));
  HIP_TRY(bufs.upload(lens, nb * 4, &lens_dev));
  if (fixed) HIP_TRY(bufs.upload(fixed, nb * L, &a.fixed));
  HIP_TRY(bufs.upload(ri.offsets.first, ri.offsets.second, &rst_offsets));
  HIP_TRY(bufs.upload(ri.i.first, ri.i.second, &rst_i));
  HIP_TRY(bufs.upload(ri.j.first, ri.j.second, &rst_j));
  HIP_TRY(bufs.upload(ri.d0.first, ri.d0.second, &rst_d0));
  HIP_TRY(bufs.upload(ri.tol.first, ri.tol.second, &rst_tol));
  HIP_TRY(bufs.upload(ri.w.first, ri.w.second, &rst_w));
  HIP_TRY(bufs.upload(state_host.data(), nb * sizeof(RelaxState), &a.state));
  HIP_TRY(bufs.zeros(n * 4, &a.x));
  HIP_TRY(bufs.alloc(n * 8, &a.Gt));
  HIP_TRY(bufs.zeros(n * 8, &a.G));
  HIP_TRY(bufs.alloc(na * 8, &coords));
  HIP_TRY(bufs.alloc(na * 8, &gc));
  HIP_TRY(bufs.alloc(nb * 8, &e_clash));
  HIP_TRY(bufs.alloc(nb * 8, &e_rst));
  HIP_TRY(bufs.alloc(nb * 8, &max_violation));
  if (trace_out) HIP_TRY(bufs.alloc((size_t)(n_iter + 1) * nb * 8, &a.trace));
  a.lens = lens_dev;
  a.e_clash = e_clash;
  a.e_rst = e_rst;
  a.L = L;
  a.F = F;
  a.angle_mask = angle_mask;
  a.move_mask = move_mask;
  a.w_tether = p.w_tether;
  a.grow = p.grow;
  a.shrink = p.shrink;
  a.max_step = p.max_step;
  const Restraints rs{rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w};
  for (int it = 0; it <= n_iter; ++it) {
    launch_nerf_scan(a.xt, lens_dev, B, L, F, fx, 0, coords, nullptr);
    launch_restraint_energy(coords, lens_dev, B, L, rs, e_rst, max_violation, gc, nullptr);
    launch_soft_clash(coords, lens_dev, B, L, p.clash_alpha, p.clash_margin, p.w_clash, e_clash, gc, nullptr);
    launch_nerf_vjp(coords, lens_dev, B, L, F, fx, 0, gc, a.xt, a.Gt, nullptr);
    a.it = it;
    a.last = it == n_iter;
    launch_relax_step(a, B, nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<float> x_host(feats_out ? n : 0);
  std::vector<double> grad_host(dfeats_out ? n : 0);
  if (feats_out) HIP_TRY(hipMemcpy(x_host.data(), a.x, n * 4, hipMemcpyDeviceToHost));
  if (dfeats_out) HIP_TRY(hipMemcpy(grad_host.data(), a.G, n * 8, hipMemcpyDeviceToHost));
  std::vector<double> trace_host(trace_out ? (size_t)(n_iter + 1) * nb : 0);
  if (trace_out) HIP_TRY(hipMemcpy(trace_host.data(), a.trace, trace_host.size() * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(state_host.data(), a.state, nb * sizeof(RelaxState), hipMemcpyDeviceToHost));
  // every download has succeeded: only now are the outputs written (the rows at or beyond a length keep what they held)
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * L * F, rows = (size_t)lens[b] * F;
    if (feats_out) memcpy(feats_out + o, x_host.data() + o, rows * 4);
    if (dfeats_out) memcpy(dfeats_out + o, grad_host.data() + o, rows * 8);
    for (int k = 0; k < 3; ++k) energy_out[3 * b + k] = state_host[b].e[k];
    if (gnorm_out) gnorm_out[b] = state_host[b].gnorm;
    if (step_io) step_io[b] = state_host[b].h;
    if (accepted_out) accepted_out[b] = state_host[b].accepted;
  }
  if (trace_out) memcpy(trace_out, trace_host.data(), trace_host.size() * 8);
  return FD_OK;
}

int fd_relax_energy(int device_id, const float* feats, const float* anchor, const int32_t* lens, int B, int L, int F,
                    const fd_relax_params* params, const uint8_t* fixed, const int32_t* rst_offsets, const int32_t* rst_i,
                    const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, double* energy_out,
                    double* gnorm_out, double* dfeats_out) {
  if (!gnorm_out) return fail(FD_E_INVALID, "null argument");
  return relax_run(device_id, feats, anchor, lens, B, L, F, params, fixed, RestraintLists{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w},
                   0, nullptr, nullptr, energy_out, gnorm_out, dfeats_out, nullptr, nullptr);
}

int fd_relax(int device_id, const float* feats, const float* anchor, const int32_t* lens, int B, int L, int F,
             const fd_relax_params* params, const uint8_t* fixed, const int32_t* rst_offsets, const int32_t* rst_i,
             const int32_t* rst_j, const double* rst_d0, const double* rst_tol, const double* rst_w, int n_iter, double* step_io,
             float* feats_out, double* energy_out, double* trace_out, int32_t* accepted_out) {
  if (!feats_out || !accepted_out) return fail(FD_E_INVALID, "null argument");
  return relax_run(device_id, feats, anchor, lens, B, L, F, params, fixed, RestraintLists{B, rst_offsets, rst_i, rst_j, rst_d0, rst_tol, rst_w},
                   n_iter, step_io, feats_out, energy_out, nullptr, nullptr, trace_out, accepted_out);
}

}  // extern "C"

// fd_symmetry_energy (descent == false: one evaluation of `pose`) and fd_symmetry_dock: the checks, the uploads, 1 + n_iter
// evaluations of two launches each, the downloads
static int symmetry_run(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* order, const double* pose,
                        const fd_symmetry_params* params, bool descent, int n_iter, double* step_io, double* pose_out, double* energy_out,
                        int32_t* contacts_out, double* wrench_out, double* dcoords_out, double* trace_out, int32_t* accepted_out) {
  if (!coords || !lens || !order || !pose || !params || !energy_out || !contacts_out) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if ((long long)B * L * 9 > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * 9 = %lld coordinates, at most 2^31 - 1", (long long)B * L * 9);
  if (int rc = check_lens(lens, B, L < kGuideMaxLen ? L : kGuideMaxLen)) return rc;
  if (int rc = check_symmetry(*params, order, pose, B)) return rc;
  if (n_iter < 0) return fail(FD_E_INVALID, "n_iter=%d must be >= 0", n_iter);
  if ((n_iter + 1LL) * B > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "(n_iter + 1) * B = %lld trace entries, at most 2^31 - 1", (n_iter + 1LL) * B);
  for (int b = 0; step_io && b < B; ++b)
    if (!(step_io[b] > 0.0) || !std::isfinite(step_io[b])) return fail(FD_E_INVALID, "step_io[%d]=%g must be > 0 and finite", b, step_io[b]);
  if (int rc = check_chain_doubles("coords", coords, lens, B, L)) return rc;
  const fd_symmetry_params& p = *params;
  const size_t na = (size_t)B * 3 * L * 3, nb = (size_t)B;
  std::vector<SymState> state_host(nb);
  for (size_t b = 0; b < nb; ++b) {
    state_host[b] = SymState{};
    memcpy(state_host[b].pose, pose + b * 12, 96);
    memcpy(state_host[b].trial, pose + b * 12, 96);  // the first trial is the input
    state_host[b].h = step_io ? step_io[b] : p.step0;
  }
  std::vector<double> rot_host((size_t)(kSymMaxOrder + 1) * 24);
  symmetry_rotations(rot_host.data());
  HIP_TRY(hipSetDevice(device_id));
  DeviceBufs bufs;
  SymPair sp{};
  SymDock sd{};
  double *e_trial, *wrench_trial, *grad = nullptr;
  int* contacts_trial;
  HIP_TRY(bufs.upload(coords, na * 8, &sp.coords));
  HIP_TRY(bufs.upload(lens, nb * 4, &sp.lens));
  HIP_TRY(bufs.upload(order, nb * 4, &sp.order));
  HIP_TRY(bufs.upload(rot_host.data(), rot_host.size() * 8, &sp.rot));
  HIP_TRY(bufs.upload(state_host.data(), nb * sizeof(SymState), &sd.state));
  HIP_TRY(bufs.alloc(nb * 24, &e_trial));
  HIP_TRY(bufs.alloc(nb * 4, &contacts_trial));
  HIP_TRY(bufs.alloc(nb * 48, &wrench_trial));
  if (dcoords_out) HIP_TRY(bufs.zeros(na * 8, &grad));  // (the launch adds: the chains with order 1 stay 0)
  if (trace_out) HIP_TRY(bufs.alloc((size_t)(n_iter + 1) * nb * 8, &sd.trace));
  sp.pose = reinterpret_cast<const double*>(sd.state) + offsetof(SymState, trial) / 8;
  sp.pose_stride = (int)(sizeof(SymState) / 8);
  sp.energy = e_trial;
  sp.contacts = contacts_trial;
  sp.wrench = wrench_trial;
  sp.dcoords = grad;
  sp.L = L;
  sp.clash_alpha = p.clash_alpha; sp.clash_margin = p.clash_margin; sp.w_clash = p.w_clash; sp.w_contact = p.w_contact;
  sp.d_on = p.d_on; sp.d_off = p.d_off; sp.w_radial = p.w_radial; sp.r_max = p.r_max;
  sd.order = sp.order;
  sd.e_trial = e_trial;
  sd.contacts_trial = contacts_trial;
  sd.wrench_trial = wrench_trial;
  sd.B = B;
  sd.lever = p.lever; sd.max_shift = p.max_shift; sd.grow = p.grow; sd.shrink = p.shrink;
  for (int it = 0; it <= n_iter; ++it) {
    launch_symmetry_pair(sp, B, nullptr);
    sd.it = it;
    sd.last = it == n_iter;
    launch_symmetry_pose(sd, nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<double> grad_host(dcoords_out ? na : 0), trace_host(trace_out ? (size_t)(n_iter + 1) * nb : 0);
  if (dcoords_out) HIP_TRY(hipMemcpy(grad_host.data(), grad, na * 8, hipMemcpyDeviceToHost));
  if (trace_out) HIP_TRY(hipMemcpy(trace_host.data(), sd.trace, trace_host.size() * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(state_host.data(), sd.state, nb * sizeof(SymState), hipMemcpyDeviceToHost));
  // every download has succeeded: only now are the outputs written
  for (size_t b = 0; b < nb; ++b) {
    const SymState& st = state_host[b];
    memcpy(energy_out + 3 * b, st.e, 24);
    contacts_out[b] = st.contacts;
    if (wrench_out) memcpy(wrench_out + 6 * b, st.wrench, 48);
    if (pose_out) memcpy(pose_out + 12 * b, st.pose, 96);
    if (descent && step_io) step_io[b] = st.h;
    if (accepted_out) accepted_out[b] = st.accepted;
  }
  if (dcoords_out) memcpy(dcoords_out, grad_host.data(), na * 8);
  if (trace_out) memcpy(trace_out, trace_host.data(), trace_host.size() * 8);
  return FD_OK;
}

extern "C" {

int fd_symmetry_energy(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* order, const double* pose,
                       const fd_symmetry_params* params, double* energy_out, int32_t* contacts_out, double* wrench_out,
                       double* dcoords_out) {
  return symmetry_run(device_id, coords, lens, B, L, order, pose, params, false, 0, nullptr, nullptr, energy_out, contacts_out, wrench_out,
                      dcoords_out, nullptr, nullptr);
}

int fd_symmetry_dock(int device_id, const double* coords, const int32_t* lens, int B, int L, const int32_t* order, const double* pose,
                     const fd_symmetry_params* params, int n_iter, double* step_io, double* pose_out, double* energy_out,
                     int32_t* contacts_out, double* trace_out, int32_t* accepted_out) {
  if (!pose_out || !accepted_out) return fail(FD_E_INVALID, "null argument");
  return symmetry_run(device_id, coords, lens, B, L, order, pose, params, true, n_iter, step_io, pose_out, energy_out, contacts_out, nullptr,
                      nullptr, trace_out, accepted_out);
}

int fd_internal_coords(int device_id, const float* xyz, const int32_t* chain_offsets, const int32_t* chain_lens, int n_chains,
                       float* feats_out) {
  if (!xyz || !chain_offsets || !chain_lens || !feats_out || n_chains < 1) return fail(FD_E_INVALID, "bad argument");
  long long n_res = 0;
  if (int rc = check_packed(chain_offsets, chain_lens, n_chains, 0x7fffffffLL / 9, &n_res)) return rc;
  const size_t nr = (size_t)n_res, nc = (size_t)n_chains;
  return device_roundtrip(device_id, {{xyz, nr * 9 * 4}, {chain_offsets, nc * 4}, {chain_lens, nc * 4}},
                          {{feats_out, nr * 9 * 4}}, [&](const RoundtripBufs& d) {
                            launch_internal_coords(d.in(0), d.in(1), d.in(2), n_chains, (int)n_res, d.out(0), nullptr);
                          });
}

int fd_superpose_rmsd(int device_id, const double* a, const double* b, const int32_t* offsets, const int32_t* lens, int n_pairs,
                      double* rmsd_out) {
  if (!a || !b || !offsets || !lens || !rmsd_out || n_pairs < 1) return fail(FD_E_INVALID, "bad argument");
  long long n_atoms = 0;
  if (int rc = check_packed(offsets, lens, n_pairs, 0x7fffffffLL / 3, &n_atoms)) return rc;
  const size_t na = (size_t)n_atoms, np = (size_t)n_pairs;
  return device_roundtrip(device_id, {{a, na * 3 * 8}, {b, na * 3 * 8}, {offsets, np * 4}, {lens, np * 4}},
                          {{rmsd_out, np * 8}}, [&](const RoundtripBufs& d) {
                            launch_superpose_rmsd(d.in(0), d.in(1), d.in(2), d.in(3), n_pairs, d.out(0), nullptr);
                          });
}

int fd_tm_score(int device_id, const double* a, const double* b, const int32_t* offsets, const int32_t* lens,
                const int32_t* norm_lens, int n_pairs, int stride, double* tm_out, double* transform_out) {
  if (!a || !b || !offsets || !lens || !tm_out) return fail(FD_E_INVALID, "null argument");
  if (n_pairs < 1) return fail(FD_E_INVALID, "n_pairs=%d must be >= 1", n_pairs);
  if (stride < 1) return fail(FD_E_INVALID, "stride=%d must be >= 1", stride);
  int max_len = 0;
  if (int rc = check_lens(lens, n_pairs, FDMI_TM_MAX_LEN, &max_len)) return rc;
  for (int p = 0; norm_lens && p < n_pairs; ++p)
    if (norm_lens[p] < lens[p])
      return fail(FD_E_INVALID, "norm_lens[%d]=%d is below lens[%d]=%d", p, norm_lens[p], p, lens[p]);
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_pairs, 0x7fffffffLL / 3, &n_res)) return rc;
  // pair p's centroids: a's at cent[6 p], b's at cent[6 p + 3]
  std::vector<double> cent((size_t)n_pairs * 6);
  if (int rc = check_coords(a, offsets, lens, n_pairs, cent.data(), 6)) return rc;
  if (int rc = check_coords(b, offsets, lens, n_pairs, cent.data() + 3, 6)) return rc;
  std::vector<int32_t> chunk_off((size_t)n_pairs + 1);
  const int n_chunks = tm_chunk_offsets(lens, n_pairs, stride, chunk_off.data());
  if (n_chunks < 0) return fail(FD_E_UNSUPPORTED, "more than 2^31 - 1 seed workgroups");
  const size_t na = (size_t)n_res, np = (size_t)n_pairs;
  return device_roundtrip(
      device_id,
      {{a, na * 3 * 8}, {b, na * 3 * 8}, {cent.data(), np * 6 * 8}, {offsets, np * 4}, {lens, np * 4},
       {norm_lens ? norm_lens : lens, np * 4}, {chunk_off.data(), (np + 1) * 4}},
      {{nullptr, tm_workspace_bytes(n_chunks)}, {tm_out, np * 8}, {transform_out, np * 12 * 8}},
      [&](const RoundtripBufs& d) {
        return launch_tm_score(d.in(0), d.in(1), d.in(2), d.in(3), d.in(4), d.in(5), d.in(6), n_pairs, n_chunks, stride,
                               max_len, d.out(0), d.out(1), d.out(2), nullptr);
      });
}

int fd_annotate_sse(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                    int8_t* sse_out, int32_t* counts_out) {
  if (!ca || !offsets || !lens || !sse_out) return fail(FD_E_INVALID, "null argument");
  if (n_chains < 1) return fail(FD_E_INVALID, "n_chains=%d must be >= 1", n_chains);
  int max_len = 0;
  if (int rc = check_lens(lens, n_chains, FDMI_SSE_MAX_LEN, &max_len)) return rc;
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_chains, 0x7fffffffLL / 3, &n_res)) return rc;
  if (int rc = check_coords(ca, offsets, lens, n_chains)) return rc;
  const size_t na = (size_t)n_res, nc = (size_t)n_chains;
  return device_roundtrip(device_id, {{ca, na * 3 * 8}, {offsets, nc * 4}, {lens, nc * 4}},
                          {{sse_out, na}, {counts_out, nc * 2 * 4}}, [&](const RoundtripBufs& d) {
                            launch_psea(d.in(0), d.in(1), d.in(2), n_chains, max_len, d.out(0), d.out(1), nullptr);
                          });
}

int fd_backbone_oxygens(int device_id, const double* nca_c, const int32_t* offsets, const int32_t* lens, int n_chains,
                        int reference_torsion, double* out) {
  if (!nca_c || !offsets || !lens || !out) return fail(FD_E_INVALID, "null argument");
  if (n_chains < 1) return fail(FD_E_INVALID, "n_chains=%d must be >= 1", n_chains);
  if (int rc = check_lens(lens, n_chains, FDMI_DSSP_MAX_LEN)) return rc;
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_chains, 0x7fffffffLL / 12, &n_res)) return rc;
  if (int rc = check_backbone(nca_c, offsets, lens, n_chains, 3)) return rc;
  const size_t nr = (size_t)n_res, nc = (size_t)n_chains;
  return device_roundtrip(device_id, {{nca_c, nr * 9 * 8}, {offsets, nc * 4}, {lens, nc * 4}}, {{out, nr * 12 * 8}},
                          [&](const RoundtripBufs& d) {
                            launch_backbone_oxygens(d.in(0), d.in(1), d.in(2), n_chains, reference_torsion, d.out(0), nullptr);
                          });
}

int fd_dssp(int device_id, const double* bb, const uint8_t* flags, const int32_t* offsets, const int32_t* lens, int n_chains,
            int8_t* state_out, int32_t* acc_out, double* energy_out, int32_t* counts_out) {
  if (!bb || !offsets || !lens || !state_out) return fail(FD_E_INVALID, "null argument");
  if ((acc_out == nullptr) != (energy_out == nullptr))
    return fail(FD_E_INVALID, "null argument: acc_out and energy_out go together");
  if (n_chains < 1) return fail(FD_E_INVALID, "n_chains=%d must be >= 1", n_chains);
  int max_len = 0;
  if (int rc = check_lens(lens, n_chains, FDMI_DSSP_MAX_LEN, &max_len)) return rc;
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_chains, 0x7fffffffLL / 12, &n_res)) return rc;
  if (int rc = check_backbone(bb, offsets, lens, n_chains, 4, 3)) return rc;
  const size_t nr = (size_t)n_res, nc = (size_t)n_chains;
  static const uint8_t no_flags = 0;
  return device_roundtrip(device_id, {{bb, nr * 12 * 8}, {offsets, nc * 4}, {lens, nc * 4}, {flags ? flags : &no_flags, flags ? nr : 1}},
                          {{state_out, nr}, {acc_out, acc_out ? nr * 2 * 4 : 4}, {energy_out, energy_out ? nr * 2 * 8 : 8},
                           {counts_out, nc * 3 * 4}},
                          [&](const RoundtripBufs& d) {
                            const unsigned char* flags_dev = d.in(3);
                            int* acc_dev = d.out(1);
                            double* energy_dev = d.out(2);
                            launch_dssp(d.in(0), flags ? flags_dev : nullptr, d.in(1), d.in(2), n_chains, max_len, d.out(0),
                                        acc_out ? acc_dev : nullptr, acc_out ? energy_dev : nullptr, d.out(3), nullptr);
                          });
}

// fd_tm_align (starts = 0: tm_align_kernel, starts 1 and 2) and fd_tm_align_ex (a bit set of starts: tm_starts_kernel)
static int tm_align_roundtrip(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                              const int32_t* pair_a, const int32_t* pair_b, const int32_t* norm_lens, int n_pairs, int max_iter,
                              double* tm_out, double* transform_out, int32_t* n_ali_out, const int64_t* map_offsets,
                              int32_t* map_out, uint32_t starts, double* start_tm_out) {
  if (!ca || !offsets || !lens || !pair_a || !pair_b || !tm_out) return fail(FD_E_INVALID, "null argument");
  if ((map_offsets == nullptr) != (map_out == nullptr))
    return fail(FD_E_INVALID, "null argument: map_offsets and map_out go together");
  if (n_chains < 1) return fail(FD_E_INVALID, "n_chains=%d must be >= 1", n_chains);
  if (n_pairs < 1) return fail(FD_E_INVALID, "n_pairs=%d must be >= 1", n_pairs);
  if (max_iter < 1) return fail(FD_E_INVALID, "max_iter=%d must be >= 1", max_iter);
  int max_len = 0;
  if (int rc = check_lens(lens, n_chains, FDMI_ALIGN_MAX_LEN, &max_len)) return rc;
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_chains, 0x7fffffffLL / 3, &n_res)) return rc;
  long long n_map = 0;
  std::vector<int32_t> norm((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    if (pair_a[p] < 0 || pair_a[p] >= n_chains || pair_b[p] < 0 || pair_b[p] >= n_chains)
      return fail(FD_E_INVALID, "pair %d = (%d, %d): chain index outside [0, %d)", p, pair_a[p], pair_b[p], n_chains);
    const int n1 = lens[pair_a[p]], n2 = lens[pair_b[p]];
    norm[p] = norm_lens ? norm_lens[p] : n2;
    if (norm[p] < std::min(n1, n2))
      return fail(FD_E_INVALID, "norm_lens[%d]=%d is below min(%d, %d)", p, norm[p], n1, n2);
    if (map_offsets && map_offsets[p] != n_map)
      return fail(FD_E_INVALID, "map_offsets[%d]=%lld, expected %lld (packed)", p, (long long)map_offsets[p], n_map);
    n_map += n1;
  }
  std::vector<double> cent((size_t)n_chains * 3);
  if (int rc = check_coords(ca, offsets, lens, n_chains, cent.data())) return rc;
  const size_t na = (size_t)n_res, nc = (size_t)n_chains, np = (size_t)n_pairs;
  const size_t map_bytes = map_out ? (size_t)n_map * 4 : 4;
  static const int64_t no_offsets = 0;
  return device_roundtrip(
      device_id,
      {{ca, na * 3 * 8}, {cent.data(), nc * 3 * 8}, {offsets, nc * 4}, {lens, nc * 4}, {pair_a, np * 4}, {pair_b, np * 4},
       {norm.data(), np * 4}, {map_offsets ? map_offsets : &no_offsets, map_offsets ? np * 8 : 8}},
      {{nullptr, na}, {nullptr, nc * 2 * 4}, {tm_out, np * 8}, {transform_out, np * 12 * 8}, {n_ali_out, np * 4},
       {map_out, map_bytes}, {start_tm_out, start_tm_out ? np * 5 * 8 : 8}},
      [&](const RoundtripBufs& d) {
        // the labels of every chain first (starts 2 and 3 read them), then the pairs; both on the null stream, in order
        launch_psea(d.in(0), d.in(2), d.in(3), n_chains, max_len, d.out(0), d.out(1), nullptr);
        const long long* map_off = d.in(7);
        int* map = d.out(5);
        double* start_tm = d.out(6);
        if (starts == 0)
          return launch_tm_align(d.in(0), d.in(1), d.in(2), d.in(3), d.out(0), d.in(4), d.in(5), d.in(6),
                                 map_out ? map_off : nullptr, n_pairs, max_iter, max_len, d.out(2), d.out(3), d.out(4),
                                 map_out ? map : nullptr, nullptr);
        return launch_tm_starts(d.in(0), d.in(1), d.in(2), d.in(3), d.out(0), d.in(4), d.in(5), d.in(6),
                                map_out ? map_off : nullptr, n_pairs, max_iter, max_len, starts, d.out(2), d.out(3), d.out(4),
                                map_out ? map : nullptr, start_tm_out ? start_tm : nullptr, nullptr);
      });
}

int fd_tm_align(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                const int32_t* pair_a, const int32_t* pair_b, const int32_t* norm_lens, int n_pairs, int max_iter,
                double* tm_out, double* transform_out, int32_t* n_ali_out, const int64_t* map_offsets, int32_t* map_out) {
  return tm_align_roundtrip(device_id, ca, offsets, lens, n_chains, pair_a, pair_b, norm_lens, n_pairs, max_iter, tm_out,
                            transform_out, n_ali_out, map_offsets, map_out, 0, nullptr);
}

int fd_tm_align_ex(int device_id, const double* ca, const int32_t* offsets, const int32_t* lens, int n_chains,
                   const int32_t* pair_a, const int32_t* pair_b, const int32_t* norm_lens, int n_pairs, int max_iter,
                   double* tm_out, double* transform_out, int32_t* n_ali_out, const int64_t* map_offsets, int32_t* map_out,
                   uint32_t starts, double* start_tm_out) {
  if (starts == 0 || starts > FDMI_ALIGN_STARTS_ALL)
    return fail(FD_E_INVALID, "starts=%u: a non-empty set of the bits 1, 2, 4, 8, 16", starts);
  return tm_align_roundtrip(device_id, ca, offsets, lens, n_chains, pair_a, pair_b, norm_lens, n_pairs, max_iter, tm_out,
                            transform_out, n_ali_out, map_offsets, map_out, starts, start_tm_out);
}

int fd_loss_terms(int device_id, const float* pred, const float* target, const int32_t* lens, int B, int L, int F,
                  const uint8_t* is_angle, float beta_ang, float beta_lin, double* sums, float* terms) {
  if (!pred || !target || !lens || !is_angle || !sums) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (F < 1 || F > 32) return fail(FD_E_INVALID, "F=%d outside [1, 32]", F);
  if (!(beta_ang > 0.f) || !(beta_lin > 0.f)) return fail(FD_E_INVALID, "beta_ang=%g beta_lin=%g must be > 0", beta_ang, beta_lin);
  if ((long long)B * L * F > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * F = %lld elements, at most 2^31 - 1", (long long)B * L * F);
  if (int rc = check_lens(lens, B, L)) return rc;
  unsigned angle_mask = 0;
  for (int f = 0; f < F; ++f)
    if (is_angle[f]) angle_mask |= 1u << f;
  const size_t n = (size_t)B * L * F;
  return device_roundtrip(device_id, {{pred, n * 4}, {target, n * 4}, {lens, (size_t)B * 4}},
                          {{sums, (size_t)B * F * 8}, {terms, terms ? n * 4 : 4}}, [&](const RoundtripBufs& d) {
                            float* terms_dev = d.out(1);
                            launch_loss_terms(d.in(0), d.in(1), d.in(2), B, L, F, angle_mask, beta_ang, beta_lin, d.out(0),
                                              terms ? terms_dev : nullptr, nullptr);
                          });
}

int fd_loss_terms_ex(int device_id, const float* pred, const float* target, const int32_t* lens, int B, int L, int F,
                     const uint8_t* is_angle, int kind, float beta_ang, float beta_lin, double* sums, float* terms,
                     int64_t* turns) {
  if (!pred || !target || !lens || !is_angle || !sums) return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (F < 1 || F > 32) return fail(FD_E_INVALID, "F=%d outside [1, 32]", F);
  if (kind != 0 && kind != 1) return fail(FD_E_INVALID, "kind=%d: 0 (smooth_l1) or 1 (l1)", kind);
  if (!(beta_ang > 0.f) || !(beta_lin > 0.f)) return fail(FD_E_INVALID, "beta_ang=%g beta_lin=%g must be > 0", beta_ang, beta_lin);
  if ((long long)B * L * F > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "B * L * F = %lld elements, at most 2^31 - 1", (long long)B * L * F);
  if (int rc = check_lens(lens, B, L)) return rc;
  unsigned angle_mask = 0;
  for (int f = 0; f < F; ++f)
    if (is_angle[f]) angle_mask |= 1u << f;
  const size_t n = (size_t)B * L * F;
  return device_roundtrip(device_id, {{pred, n * 4}, {target, n * 4}, {lens, (size_t)B * 4}},
                          {{sums, (size_t)B * F * 8}, {terms, terms ? n * 4 : 4}, {turns, turns ? (size_t)B * F * 8 : 8}},
                          [&](const RoundtripBufs& d) {
                            float* terms_dev = d.out(1);
                            long long* turns_dev = d.out(2);
                            launch_loss_terms_ex(d.in(0), d.in(1), d.in(2), B, L, F, angle_mask, kind, beta_ang, beta_lin, d.out(0),
                                                 terms ? terms_dev : nullptr, turns ? turns_dev : nullptr, nullptr);
                          });
}

int fd_pairwise_dist(int device_id, const float* angles, const float* corrupted, const float* pred, const float* keep,
                     const float* spread, const float* coef, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                     double* sums, int64_t* pairs, double* ca_out) {
  if (!angles || !corrupted || !pred || !keep || !spread || !lens || !feat_idx || !sums || !pairs)
    return fail(FD_E_INVALID, "null argument");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (F < 6 || F > 32) return fail(FD_E_INVALID, "F=%d outside [6, 32]", F);
  if (int rc = check_pairwise(keep, coef, feat_idx, B, L, F)) return rc;
  if (int rc = check_lens(lens, B, L)) return rc;
  const PairwiseFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5]};
  const size_t n = (size_t)B * L * F, nb = (size_t)B;
  static const float no_coef = 1.f;
  return device_roundtrip(device_id,
                          {{angles, n * 4}, {corrupted, n * 4}, {pred, n * 4}, {keep, nb * 4}, {spread, nb * 4},
                           {coef ? coef : &no_coef, coef ? nb * 4 : 4}, {lens, nb * 4}},
                          {{sums, nb * 8}, {pairs, nb * 8}, {ca_out, ca_out ? nb * 2 * L * 3 * 8 : 8}},
                          [&](const RoundtripBufs& d) {
                            const float* coef_dev = d.in(5);
                            double* ca_dev = d.out(2);
                            launch_pairwise_dist(d.in(0), d.in(1), d.in(2), d.in(3), d.in(4), coef ? coef_dev : nullptr, d.in(6),
                                                 B, L, F, fx, d.out(0), d.out(1), ca_out ? ca_dev : nullptr, nullptr);
                          });
}

int fd_backbone_clashes(int device_id, const float* xyz, const int32_t* chain_offsets, const int32_t* chain_lens,
                        int n_chains, double alpha, int32_t* counts_out, uint8_t* flags_out) {
  if (!xyz || !chain_offsets || !chain_lens || !counts_out) return fail(FD_E_INVALID, "null argument");
  if (n_chains < 1) return fail(FD_E_INVALID, "n_chains=%d must be >= 1", n_chains);
  if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(FD_E_INVALID, "alpha=%g must be > 0 and finite", alpha);
  long long n_res = 0;
  if (int rc = check_packed(chain_offsets, chain_lens, n_chains, 0x7fffffffLL / 9, &n_res)) return rc;
  if (int rc = check_atom_cap(chain_lens, n_chains, 3)) return rc;
  if (int rc = check_coords_f32(xyz, chain_offsets, chain_lens, n_chains, 3)) return rc;
  const size_t nr = (size_t)n_res, nc = (size_t)n_chains;
  return device_roundtrip(device_id, {{xyz, nr * 9 * 4}, {chain_offsets, nc * 4}, {chain_lens, nc * 4}},
                          {{counts_out, nc * 4}, {flags_out, flags_out ? nr * 3 : 4}}, [&](const RoundtripBufs& d) {
                            unsigned char* flags_dev = d.out(1);
                            launch_backbone_clashes(d.in(0), d.in(1), d.in(2), n_chains, alpha, d.out(0),
                                                    flags_out ? flags_dev : nullptr, nullptr);
                          });
}

int fd_lddt(int device_id, const float* model, const float* ref, const int32_t* offsets, const int32_t* lens, int n_pairs,
            int atoms_per_res, double radius, const double* thresholds, int n_thresholds, int64_t* counts_out,
            int32_t* res_counts_out) {
  if (!model || !ref || !offsets || !lens || !thresholds || !counts_out) return fail(FD_E_INVALID, "null argument");
  if (n_pairs < 1) return fail(FD_E_INVALID, "n_pairs=%d must be >= 1", n_pairs);
  if (atoms_per_res < 1 || atoms_per_res > 8) return fail(FD_E_INVALID, "atoms_per_res=%d outside [1, 8]", atoms_per_res);
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(FD_E_INVALID, "radius=%g must be > 0 and finite", radius);
  if (n_thresholds < 1 || n_thresholds > kLddtMaxThresholds)
    return fail(FD_E_INVALID, "n_thresholds=%d outside [1, %d]", n_thresholds, kLddtMaxThresholds);
  LddtThresholds thr{};   // unused places stay 0: no pair passes them
  for (int k = 0; k < n_thresholds; ++k) {
    if (!(thresholds[k] > 0.0) || !std::isfinite(thresholds[k]))
      return fail(FD_E_INVALID, "thresholds[%d]=%g must be > 0 and finite", k, thresholds[k]);
    thr.t[k] = thresholds[k];
  }
  const int A = atoms_per_res;
  long long n_res = 0;
  if (int rc = check_packed(offsets, lens, n_pairs, 0x7fffffffLL / (3 * A), &n_res)) return rc;
  if (int rc = check_atom_cap(lens, n_pairs, A)) return rc;
  if (int rc = check_coords_f32(model, offsets, lens, n_pairs, A)) return rc;
  if (int rc = check_coords_f32(ref, offsets, lens, n_pairs, A)) return rc;
  const size_t nr = (size_t)n_res, np = (size_t)n_pairs;
  return device_roundtrip(device_id, {{model, nr * A * 3 * 4}, {ref, nr * A * 3 * 4}, {offsets, np * 4}, {lens, np * 4}},
                          {{counts_out, np * 2 * 8}, {res_counts_out, res_counts_out ? nr * 2 * 4 : 4}},
                          [&](const RoundtripBufs& d) {
                            int* res_dev = d.out(1);
                            launch_lddt(d.in(0), d.in(1), d.in(2), d.in(3), n_pairs, A, radius, thr, d.out(0),
                                        res_counts_out ? res_dev : nullptr, nullptr);
                          });
}

int fd_steer_rewards(int device_id, const float* x, const int32_t* lens, int B, int L, int F, const int32_t* feat_idx,
                     const float* offset, const uint8_t* is_angle, const double* weights, double clash_alpha,
                     double* terms_out, double* reward_out) {
  if (!x || !lens || !feat_idx || !weights || !terms_out || !reward_out) return fail(FD_E_INVALID, "null argument");
  if (offset && !is_angle) return fail(FD_E_INVALID, "null argument: an offset needs is_angle");
  if (B < 1 || L < 1) return fail(FD_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (int rc = check_steer(lens, B, L, F, feat_idx, weights, clash_alpha, offset)) return rc;
  for (int b = 0; b < B; ++b)
    for (size_t i = (size_t)b * L * F; i < ((size_t)b * L + lens[b]) * F; ++i)
      if (!std::isfinite(x[i])) return fail(FD_E_INVALID, "x is not finite at sequence %d, position %d", b, (int)(i / F - (size_t)b * L));
  const NerfFeatures fx{feat_idx[0], feat_idx[1], feat_idx[2], feat_idx[3], feat_idx[4], feat_idx[5], feat_idx[6], feat_idx[7], feat_idx[8]};
  SteerOffset off{};
  SteerWeights wt{};
  unsigned angle_mask = 0;
  int max_len = 0;
  std::vector<int32_t> offsets((size_t)B);
  for (int b = 0; b < B; ++b) {
    offsets[b] = b * L;
    max_len = std::max(max_len, (int)lens[b]);
  }
  for (int k = 0; k < 4; ++k) wt.w[k] = weights[k];
  off.has_offset = offset ? 1 : 0;
  for (int f = 0; offset && f < F; ++f) {
    off.offset[f] = offset[f];
    if (is_angle[f]) angle_mask |= 1u << f;
  }
  const size_t n = (size_t)B * L * F, nr = (size_t)B * L, nb = (size_t)B;
  return device_roundtrip(device_id, {{x, n * 4}, {lens, nb * 4}, {offsets.data(), nb * 4}},
                          {{nullptr, n * 4}, {nullptr, nr * 9 * 8}, {nullptr, nr * 9 * 4}, {nullptr, nr * 3 * 8}, {nullptr, nr},
                           {nullptr, nb * 2 * 4}, {nullptr, nb * 4}, {terms_out, nb * 4 * 8}, {reward_out, nb * 8}},
                          [&](const RoundtripBufs& d) {
                            float* ang = d.out(0);
                            const SteerWork wk{d.out(1), d.out(2), d.out(3), d.out(4), d.out(5), d.out(6), d.in(2)};
                            launch_steer_shift(d.in(0), d.in(1), B, L, F, off, angle_mask, ang, nullptr);
                            launch_steer_rewards(ang, d.in(1), B, L, F, fx, wt, clash_alpha, max_len, wk, d.out(7), d.out(8), nullptr);
                          });
}

int fd_steer_resample(int device_id, const double* reward, double* logw, double* r_prev, int G, int P, double lambda,
                      double ess_frac, const double* u, int32_t* ancestors_out, uint8_t* resampled_out) {
  if (!reward || !logw || !r_prev || !u || !ancestors_out || !resampled_out) return fail(FD_E_INVALID, "null argument");
  if (G < 1) return fail(FD_E_INVALID, "G=%d must be >= 1", G);
  if (P < 1 || P > kSteerMaxParticles) return fail(FD_E_INVALID, "P=%d outside [1, %d]", P, kSteerMaxParticles);
  if ((long long)G * P > 0x7fffffffLL) return fail(FD_E_UNSUPPORTED, "G * P = %lld particles, at most 2^31 - 1", (long long)G * P);
  if (!std::isfinite(lambda)) return fail(FD_E_INVALID, "lambda=%g must be finite", lambda);
  if (!(ess_frac >= 0.0)) return fail(FD_E_INVALID, "ess_frac=%g must be >= 0", ess_frac);
  if (int rc = check_steer_u(u, (size_t)G)) return rc;
  const size_t nb = (size_t)G * P;
  return device_roundtrip(device_id, {{reward, nb * 8}, {logw, nb * 8}, {r_prev, nb * 8}, {u, (size_t)G * 8}},
                          {{logw, nb * 8}, {r_prev, nb * 8}, {ancestors_out, nb * 4}, {resampled_out, (size_t)G}},
                          [&](const RoundtripBufs& d) -> hipError_t {
                            double *logw_dev = d.out(0), *r_prev_dev = d.out(1);
                            const double *logw_in = d.in(1), *r_prev_in = d.in(2);
                            if (hipError_t e = hipMemcpyAsync(logw_dev, logw_in, nb * 8, hipMemcpyDeviceToDevice, nullptr)) return e;
                            if (hipError_t e = hipMemcpyAsync(r_prev_dev, r_prev_in, nb * 8, hipMemcpyDeviceToDevice, nullptr)) return e;
                            launch_steer_resample(d.in(0), logw_dev, r_prev_dev, G, P, lambda, ess_frac, d.in(3), d.out(2), d.out(3),
                                                  nullptr);
                            return hipSuccess;
                          });
}

// rows of non-decreasing edges without a NaN: edges[rows][nbins + 1]
static int check_edges(const double* edges, long long rows, int nbins) {
  for (long long r = 0; r < rows; ++r) {
    const double* e = edges + r * (nbins + 1);
    for (int i = 0; i <= nbins; ++i)
      if (std::isnan(e[i]) || (i > 0 && e[i] < e[i - 1]))
        return fail(FD_E_INVALID, "edges: row %lld is decreasing or NaN at %d (%g)", r, i, e[i]);
  }
  return FD_OK;
}

static int check_hist_shape(int64_t N, int F, int nbins) {
  if (N < 1 || N > 0x7fffffffLL) return fail(FD_E_INVALID, "N=%lld outside [1, 2^31 - 1]", (long long)N);
  if (F < 1 || F > 32) return fail(FD_E_INVALID, "F=%d outside [1, 32]", F);
  if (nbins < 1 || nbins > FDMI_HIST_MAX_BINS) return fail(FD_E_INVALID, "nbins=%d outside [1, %d]", nbins, FDMI_HIST_MAX_BINS);
  return FD_OK;
}

int fd_hist_columns(int device_id, const float* values, int64_t N, int F, const double* edges, int nbins,
                    const uint8_t* rows_valid, int64_t* counts, int64_t* outside) {
  if (!values || !edges || !counts || !outside) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_hist_shape(N, F, nbins)) return rc;
  if (int rc = check_edges(edges, F, nbins)) return rc;
  const size_t n = (size_t)N, nf = (size_t)F, count_bytes = nf * nbins * 8;
  static const uint8_t no_rows = 1;
  return device_roundtrip(device_id, {{values, n * nf * 4}, {edges, nf * (nbins + 1) * 8}, {rows_valid ? rows_valid : &no_rows, rows_valid ? n : 1}},
                          {{counts, count_bytes}, {outside, nf * 8}}, [&](const RoundtripBufs& d) -> hipError_t {
                            unsigned long long *counts_dev = d.out(0), *outside_dev = d.out(1);
                            const unsigned char* valid_dev = d.in(2);
                            if (hipError_t e = hipMemsetAsync(counts_dev, 0, count_bytes, nullptr)) return e;
                            if (hipError_t e = hipMemsetAsync(outside_dev, 0, nf * 8, nullptr)) return e;
                            launch_hist_columns(d.in(0), N, F, d.in(1), nbins, rows_valid ? valid_dev : nullptr, counts_dev,
                                                outside_dev, nullptr);
                            return hipSuccess;
                          });
}

// the arguments fd_noise_minmax and fd_noise_hist share
static int check_noise(const float* x0, int64_t N, int F, const uint8_t* is_angle, const float* scale, const float* keep,
                       const float* spread, int T, const int32_t* timesteps, int nT, const float* eps_in, const float* cmp_in,
                       unsigned* angle_mask) {
  if (!x0 || !is_angle || !scale || !keep || !spread || !timesteps) return fail(FD_E_INVALID, "null argument");
  if ((eps_in == nullptr) != (cmp_in == nullptr)) return fail(FD_E_INVALID, "null argument: eps_in and cmp_in go together");
  if (int rc = check_hist_shape(N, F, 1)) return rc;
  if (T < 1) return fail(FD_E_INVALID, "T=%d must be >= 1", T);
  if (nT < 1 || nT > 65535) return fail(FD_E_INVALID, "nT=%d outside [1, 65535]", nT);
  for (int i = 0; i < nT; ++i)
    if (timesteps[i] < 0 || timesteps[i] >= T) return fail(FD_E_INVALID, "timesteps[%d]=%d outside [0, %d)", i, timesteps[i], T);
  for (int t = 0; t < T; ++t)
    if (!std::isfinite(keep[t]) || !std::isfinite(spread[t]))
      return fail(FD_E_INVALID, "keep[%d]=%g spread[%d]=%g must be finite", t, (double)keep[t], t, (double)spread[t]);
  *angle_mask = 0;
  for (int f = 0; f < F; ++f) {
    if (!std::isfinite(scale[f])) return fail(FD_E_INVALID, "scale[%d]=%g must be finite", f, (double)scale[f]);
    if (is_angle[f]) *angle_mask |= 1u << f;
  }
  return FD_OK;
}

int fd_noise_minmax(int device_id, const float* x0, int64_t N, int F, const uint8_t* is_angle, const float* scale,
                    const float* keep, const float* spread, int T, const int32_t* timesteps, int nT, uint64_t seed_eps,
                    uint64_t seed_cmp, int64_t row_offset, const float* eps_in, const float* cmp_in, float* minmax_out) {
  unsigned angle_mask = 0;
  if (int rc = check_noise(x0, N, F, is_angle, scale, keep, spread, T, timesteps, nT, eps_in, cmp_in, &angle_mask)) return rc;
  if (!minmax_out) return fail(FD_E_INVALID, "null argument");
  const size_t n = (size_t)N * F, draws = (size_t)nT * n * 4, keys = (size_t)nT * 2 * F;
  static const float no_draws = 0.f;
  std::vector<uint32_t> mins(keys), maxs(keys);
  const int rc = device_roundtrip(
      device_id,
      {{x0, n * 4}, {scale, (size_t)F * 4}, {keep, (size_t)T * 4}, {spread, (size_t)T * 4}, {timesteps, (size_t)nT * 4},
       {eps_in ? eps_in : &no_draws, eps_in ? draws : 4}, {cmp_in ? cmp_in : &no_draws, cmp_in ? draws : 4}},
      {{mins.data(), keys * 4}, {maxs.data(), keys * 4}}, [&](const RoundtripBufs& d) -> hipError_t {
        unsigned *mins_dev = d.out(0), *maxs_dev = d.out(1);
        const float *eps_dev = d.in(5), *cmp_dev = d.in(6);
        if (hipError_t e = hipMemsetAsync(mins_dev, 0xff, keys * 4, nullptr)) return e;
        if (hipError_t e = hipMemsetAsync(maxs_dev, 0, keys * 4, nullptr)) return e;
        const NoiseArgs a{d.in(0), d.in(1), d.in(2), d.in(3), d.in(4), eps_in ? eps_dev : nullptr, cmp_in ? cmp_dev : nullptr,
                          (long long)N, (long long)row_offset, F, 4, angle_mask, seed_eps, seed_cmp};
        launch_noise_minmax(a, nT, mins_dev, maxs_dev, nullptr);
        return hipSuccess;
      });
  if (rc != FD_OK) return rc;
  // the kernel's order-preserving keys back to floats
  auto value = [](uint32_t key) {
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    float v;
    memcpy(&v, &bits, 4);
    return v;
  };
  for (size_t k = 0; k < keys; ++k) {
    minmax_out[2 * k] = value(mins[k]);
    minmax_out[2 * k + 1] = value(maxs[k]);
  }
  return FD_OK;
}

int fd_noise_hist(int device_id, const float* x0, int64_t N, int F, const uint8_t* is_angle, const float* scale,
                  const float* keep, const float* spread, int T, const int32_t* timesteps, int nT, uint64_t seed_eps,
                  uint64_t seed_cmp, int64_t row_offset, const float* eps_in, const float* cmp_in, const double* edges,
                  int nbins, int64_t* counts, int64_t* outside, float* x_t_out, float* cmp_out, float* eps_out) {
  unsigned angle_mask = 0;
  if (int rc = check_noise(x0, N, F, is_angle, scale, keep, spread, T, timesteps, nT, eps_in, cmp_in, &angle_mask)) return rc;
  if (!edges || !counts || !outside) return fail(FD_E_INVALID, "null argument");
  if (int rc = check_hist_shape(N, F, nbins)) return rc;
  if (int rc = check_edges(edges, (long long)nT * F, nbins)) return rc;
  const size_t n = (size_t)N * F, draws = (size_t)nT * n * 4, slabs = (size_t)nT * 2 * F, count_bytes = slabs * nbins * 8;
  static const float no_draws = 0.f;
  return device_roundtrip(
      device_id,
      {{x0, n * 4}, {scale, (size_t)F * 4}, {keep, (size_t)T * 4}, {spread, (size_t)T * 4}, {timesteps, (size_t)nT * 4},
       {eps_in ? eps_in : &no_draws, eps_in ? draws : 4}, {cmp_in ? cmp_in : &no_draws, cmp_in ? draws : 4},
       {edges, (size_t)nT * F * (nbins + 1) * 8}},
      {{counts, count_bytes}, {outside, slabs * 8}, {x_t_out, x_t_out ? draws : 4}, {cmp_out, cmp_out ? draws : 4},
       {eps_out, eps_out ? draws : 4}},
      [&](const RoundtripBufs& d) -> hipError_t {
        unsigned long long *counts_dev = d.out(0), *outside_dev = d.out(1);
        float *x_t_dev = d.out(2), *cmp_out_dev = d.out(3), *eps_out_dev = d.out(4);
        const float *eps_dev = d.in(5), *cmp_dev = d.in(6);
        if (hipError_t e = hipMemsetAsync(counts_dev, 0, count_bytes, nullptr)) return e;
        if (hipError_t e = hipMemsetAsync(outside_dev, 0, slabs * 8, nullptr)) return e;
        const NoiseArgs a{d.in(0), d.in(1), d.in(2), d.in(3), d.in(4), eps_in ? eps_dev : nullptr, cmp_in ? cmp_dev : nullptr,
                          (long long)N, (long long)row_offset, F, noise_features_per_group(nbins), angle_mask, seed_eps, seed_cmp};
        launch_noise_hist(a, nT, d.in(7), nbins, counts_dev, outside_dev, x_t_out ? x_t_dev : nullptr,
                          cmp_out ? cmp_out_dev : nullptr, eps_out ? eps_out_dev : nullptr, nullptr);
        return hipSuccess;
      });
}

}  // extern "C"
