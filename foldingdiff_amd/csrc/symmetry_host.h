// Host-only: what the guided symmetry entries (fd_scaffold_guide_step_sym in api_structures.hip, fd_sample_guided_inpaint_sym in
// api_run.hip) stage for launch_symmetry_guide (symmetry.hip) into buffers of the call's lifetime.
#pragma once
#include <cstring>
#include <vector>

#include "fdmi_kernels.h"
#include "host_common.h"

namespace fdmi {

// check_symmetry has passed and a chain has an order above 1.  The descent's state starts from pose_in and step (null: step0);
// the fit's lists name every atom of the chains with an order above 1, with unit weights.  placed_in ([B][3L][3] on the host)
// not null: the fit's targets are uploaded from it; carried: a packed target buffer is allocated that the statement's placement
// refills for the visit after (g->fit.xyz stays null: the caller sets it to g->placed_packed behind the first visit); neither:
// no fit.  g->placed is the caller's.
inline int stage_symmetry_guide(DeviceBufs* bufs, const int32_t* order, const double* pose_in, const double* step,
                                const fd_symmetry_params& q, const int32_t* lens, const int* lens_dev, const double* coords_dev, int B, int L,
                                const double* placed_in, bool carried, SymGuide* g) {
  const size_t nb = (size_t)B;
  std::vector<SymState> state(nb);
  std::vector<int32_t> fit_offsets(nb + 1, 0), fit_atom;
  for (size_t b = 0; b < nb; ++b) {
    state[b] = SymState{};
    memcpy(state[b].pose, pose_in + b * 12, 96);
    memcpy(state[b].trial, pose_in + b * 12, 96);
    state[b].h = step ? step[b] : q.step0;
    const int na_b = order[b] >= 2 ? 3 * lens[b] : 0;
    fit_offsets[b + 1] = fit_offsets[b] + na_b;
    for (int a = 0; a < na_b; ++a) fit_atom.push_back(a);
  }
  std::vector<double> rot((size_t)(kSymMaxOrder + 1) * 24), fit_w(fit_atom.size(), 1.0);
  symmetry_rotations(rot.data());
  HIP_TRY(bufs->upload(order, nb * 4, &g->pair.order));
  HIP_TRY(bufs->upload(rot.data(), rot.size() * 8, &g->pair.rot));
  HIP_TRY(bufs->upload(state.data(), nb * sizeof(SymState), &g->dock.state));
  if (placed_in || carried) {
    HIP_TRY(bufs->upload(fit_offsets.data(), (nb + 1) * 4, &g->fit.offsets));
    HIP_TRY(bufs->upload(fit_atom.data(), fit_atom.size() * 4, &g->fit.atom));
    HIP_TRY(bufs->upload(fit_w.data(), fit_w.size() * 8, &g->fit.w));
    HIP_TRY(bufs->alloc(nb * 8, &g->fit_energy));
    HIP_TRY(bufs->alloc(nb * 8, &g->fit_rmsd));
    HIP_TRY(bufs->alloc(nb * 96, &g->fit_transform));
  }
  if (placed_in) {  // the placed atoms of the chains with an order above 1, packed
    std::vector<double> fit_xyz(fit_atom.size() * 3);
    for (size_t b = 0; b < nb; ++b)
      memcpy(fit_xyz.data() + (size_t)fit_offsets[b] * 3, placed_in + b * 3 * L * 3, (size_t)(fit_offsets[b + 1] - fit_offsets[b]) * 24);
    HIP_TRY(bufs->upload(fit_xyz.data(), fit_xyz.size() * 8, &g->fit.xyz));
  }
  if (carried) HIP_TRY(bufs->alloc(fit_atom.size() * 24, &g->placed_packed));
  HIP_TRY(bufs->alloc(nb * 3 * L * 3 * 8, &g->g_spare));
  HIP_TRY(bufs->alloc(nb * 24, &g->e_trial));
  HIP_TRY(bufs->alloc(nb * 48, &g->wrench_trial));
  HIP_TRY(bufs->alloc(nb * 4, &g->contacts_trial));
  HIP_TRY(bufs->alloc(nb * 24, &g->energy));
  HIP_TRY(bufs->alloc(nb * 4, &g->contacts));
  g->pair.coords = coords_dev;
  g->pair.lens = lens_dev;
  g->pair.L = L;
  g->pair.clash_alpha = q.clash_alpha; g->pair.clash_margin = q.clash_margin; g->pair.w_clash = q.w_clash; g->pair.w_contact = q.w_contact;
  g->pair.d_on = q.d_on; g->pair.d_off = q.d_off; g->pair.w_radial = q.w_radial; g->pair.r_max = q.r_max;
  g->dock.B = B;
  g->dock.order = g->pair.order;
  g->dock.lever = q.lever; g->dock.max_shift = q.max_shift; g->dock.grow = q.grow; g->dock.shrink = q.shrink;
  g->pose_iters = q.pose_iters;
  return FD_OK;
}

}  // namespace fdmi
