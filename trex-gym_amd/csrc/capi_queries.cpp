// C-ABI of include/trex_batch.h, the queries: every call that only reads the batch's state and writes caller buffers, and the setters
// of the tables such calls read (link probes, proximity shapes) - and the reward terms, which read the state likewise and keep a
// history of their own in the batch. Nothing here changes what a step launch does; that is capi.cpp.
#include <cstring>
#include <type_traits>

#include "batch.hpp"
#include "dynamics.h"
#include "inverse_kinematics.h"
#include "observation.h"
#include "proximity.h"
#include "raycast.h"
#include "render.h"
#include "reward.h"
#include "step_launch.h"
#include "termination.h"

namespace {

template <class A, class = void> struct has_qd : std::false_type {};
template <class A> struct has_qd<A, std::void_t<decltype(A::qd)>> : std::true_type {};
template <class A, class = void> struct has_n_envs : std::false_type {};
template <class A> struct has_n_envs<A, std::void_t<decltype(A::n_envs)>> : std::true_type {};
// the argument struct of a query launch, zeroed, with the model and the state of the batch (qd, n_envs: where the struct has them)
template <class A> A query_args(const TrexBatch *b) {
  A a{};
  a.model = b->dmodel; a.base = b->arr.base; a.q = b->arr.q;
  if constexpr (has_qd<A>::value) a.qd = b->arr.qd;
  if constexpr (has_n_envs<A>::value) a.n_envs = b->n;
  return a;
}

// `link` of the call `who` must lie in [lo, number of URDF links)
int check_link(const TrexBatch *b, const char *who, int link, int lo) {
  if (link >= lo && link < (int)b->links.body.size()) return TREX_OK;
  return fail(TREX_E_INVALID, std::string(who) + ": link " + std::to_string(link) + " out of range [" + std::to_string(lo) + ", " +
                                  std::to_string(b->links.body.size()) + ")");
}

// `set` of the call `who` must be a probe set of the batch that holds probes
int check_probe_set(const TrexBatch *b, const char *who, int set) {
  if (set < 0 || set >= TREX_LINK_SETS)
    return fail(TREX_E_INVALID, std::string(who) + ": set " + std::to_string(set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ")");
  if (b->probes[set].n < 1)
    return fail(TREX_E_INVALID, std::string(who) + ": probe set " + std::to_string(set) + " is empty (trex_batch_set_link_probes)");
  return TREX_OK;
}

}  // namespace

extern "C" {

int trex_batch_head_position(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)b->n * 3 * sizeof(float), "trex_batch_head_position: out");
  HIP_TRY(trex_launch_head(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_link_transforms(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)b->n * b->arr.num_links * 7 * sizeof(float), "trex_batch_link_transforms: out");
  HIP_TRY(trex_launch_link_transforms(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream, 0));
  return TREX_OK;
}

int trex_batch_visual_transforms(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "out is null");
  if (b->arr.num_visuals == 0) return fail(TREX_E_INVALID, "the model has no <visual> meshes");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)b->n * b->arr.num_visuals * 7 * sizeof(float), "trex_batch_visual_transforms: out");
  HIP_TRY(trex_launch_link_transforms(b->dmodel, b->arr, b->n, out_dev, (hipStream_t)stream, 1));
  return TREX_OK;
}

int trex_batch_contact_wrench(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!b->sens_on) return fail(TREX_E_INVALID, "trex_batch_contact_wrench: the contact sensor is off (trex_batch_set_contact_sensor)");
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_contact_wrench: out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)b->n * b->nb * 6 * sizeof(float), "trex_batch_contact_wrench: out");
  HIP_TRY(trex_launch_contact_wrench(b->sens.as<float>(), out_dev, b->n, b->nb, (hipStream_t)stream));
  return TREX_OK;
}

// ---- dynamics queries (dynamics.hip): read the state, write only their outputs; nothing allocated, nothing waited for
static TrexDynArgs dyn_args(const TrexBatch *b, float *out) {
  TrexDynArgs a = query_args<TrexDynArgs>(b);
  a.mass_scale = b->arr.domain ? b->arr.mass_scale : nullptr;
  a.nb = b->nb; a.out = out;
  return a;
}

int trex_batch_inverse_dynamics(TrexBatch *b, const float *accel_dev, float *force_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!force_dev) return fail(TREX_E_INVALID, "trex_batch_inverse_dynamics: force is null");
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * (6 + b->nj) * sizeof(float);
  BUF_TRY(b, accel_dev, bytes, "trex_batch_inverse_dynamics: accel");
  BUF_TRY(b, force_dev, bytes, "trex_batch_inverse_dynamics: force");
  TrexDynArgs a = dyn_args(b, force_dev);
  a.accel = accel_dev;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_INVERSE_DYNAMICS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_mass_matrix(TrexBatch *b, float *M_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!M_dev) return fail(TREX_E_INVALID, "trex_batch_mass_matrix: M is null");
  DeviceGuard guard(b->device);
  const size_t D = 6 + (size_t)b->nj;
  BUF_TRY(b, M_dev, (size_t)b->n * D * D * sizeof(float), "trex_batch_mass_matrix: M");
  HIP_TRY(trex_launch_dynamics(dyn_args(b, M_dev), TREX_DYN_MASS_MATRIX, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_jacobian(TrexBatch *b, int link, const double local_xyz[3], float *J_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!J_dev || !local_xyz) return fail(TREX_E_INVALID, "trex_batch_jacobian: null argument");
  if (int c = check_link(b, "trex_batch_jacobian", link, 0)) return c;
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(local_xyz[c])) return fail(TREX_E_INVALID, "trex_batch_jacobian: local_xyz is not finite");
  DeviceGuard guard(b->device);
  BUF_TRY(b, J_dev, (size_t)b->n * 6 * (6 + b->nj) * sizeof(float), "trex_batch_jacobian: J");
  TrexDynArgs a = dyn_args(b, J_dev);
  const trex::LinkPoint p = trex::link_point(b->links, link, local_xyz);   // the point in the frame of the link's body
  a.jac_body = p.body;
  std::memcpy(a.jac_point, p.point, sizeof p.point);
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_JACOBIAN, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_centroidal(TrexBatch *b, float *out_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!out_dev) return fail(TREX_E_INVALID, "trex_batch_centroidal: out is null");
  DeviceGuard guard(b->device);
  BUF_TRY(b, out_dev, (size_t)b->n * TREX_DYN_CENT_FLOATS * sizeof(float), "trex_batch_centroidal: out");
  HIP_TRY(trex_launch_dynamics(dyn_args(b, out_dev), TREX_DYN_CENTROIDAL, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_forward_dynamics(TrexBatch *b, const float *force_dev, float *accel_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!accel_dev) return fail(TREX_E_INVALID, "trex_batch_forward_dynamics: accel is null");
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * (6 + b->nj) * sizeof(float);
  BUF_TRY(b, force_dev, bytes, "trex_batch_forward_dynamics: force");
  BUF_TRY(b, accel_dev, bytes, "trex_batch_forward_dynamics: accel");
  TrexDynArgs a = dyn_args(b, accel_dev);
  a.rhs = force_dev;
  a.num_rhs = 1;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_FORWARD_DYNAMICS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_solve_mass(TrexBatch *b, const float *rhs_dev, int num_rhs, float *x_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!x_dev) return fail(TREX_E_INVALID, "trex_batch_solve_mass: x is null");
  if (num_rhs < 1 || num_rhs > TREX_DYN_MAX_RHS)
    return fail(TREX_E_INVALID, "trex_batch_solve_mass: num_rhs " + std::to_string(num_rhs) + " outside 1.." + std::to_string(TREX_DYN_MAX_RHS));
  if (!rhs_dev && num_rhs != 6 + b->nj)
    return fail(TREX_E_INVALID, "trex_batch_solve_mass: a null rhs is the identity, num_rhs must be " + std::to_string(6 + b->nj));
  DeviceGuard guard(b->device);
  const size_t bytes = (size_t)b->n * num_rhs * (6 + b->nj) * sizeof(float);
  BUF_TRY(b, rhs_dev, bytes, "trex_batch_solve_mass: rhs");
  BUF_TRY(b, x_dev, bytes, "trex_batch_solve_mass: x");
  TrexDynArgs a = dyn_args(b, x_dev);
  a.rhs = rhs_dev;
  a.num_rhs = num_rhs;
  HIP_TRY(trex_launch_dynamics(a, TREX_DYN_SOLVE_MASS, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_contact_stats(TrexBatch *b, int32_t *count_dev, float *normal_impulse_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  DeviceGuard guard(b->device);
  BUF_TRY(b, count_dev, (size_t)b->n * sizeof(int32_t), "trex_batch_contact_stats: count");
  BUF_TRY(b, normal_impulse_dev, (size_t)b->n * sizeof(float), "trex_batch_contact_stats: normal_impulse");
  if (count_dev || normal_impulse_dev)
    HIP_TRY(trex_launch_scalars_get(b->arr, b->n, count_dev, normal_impulse_dev, nullptr, (hipStream_t)stream));
  return TREX_OK;
}

// The primitive / plane table the renderer and the ray casts share (render.cpp), once per batch and made by whichever call comes
// first (trex_model_load stays as fast as it was). `who`: the calling entry point, for the message.
static int ensure_render_table(TrexBatch *b, const char *who) {
  if (b->render_prim) return TREX_OK;
  trex::HostModel hm;
  hm.nb = b->nb;
  hm.hull_xyz = b->hull_xyz; hm.hull_radius = b->hull_radius; hm.hull_start = b->hull_start; hm.hull_group_start = b->hull_group_start;
  std::vector<TrexRenderPrim> prims;
  std::vector<float> planes;
  const int np = trex::render_table(hm, prims, planes);
  if (np > TREX_RENDER_MAXPRIM)
    return fail(TREX_E_UNSUPPORTED, std::string(who) + ": the model has " + std::to_string(np) + " drawable primitives, the renderer " +
                                        std::to_string(TREX_RENDER_MAXPRIM));
  if (planes.empty()) planes.assign(4, 0.f);
  if (prims.empty()) prims.resize(1);
  DeviceBuf pp, pl;
  HIP_TRY(pp.alloc(prims.size() * sizeof(TrexRenderPrim), false));
  HIP_TRY(pl.alloc(planes.size() * sizeof(float), false));
  HIP_TRY(hipMemcpy(pp.p, prims.data(), pp.bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pl.p, planes.data(), pl.bytes, hipMemcpyHostToDevice));
  b->render_prim = std::move(pp); b->render_plane = std::move(pl); b->render_nprim = np;
  return TREX_OK;
}

int trex_batch_render(TrexBatch *b, const TrexCamera *cam, int width, int height, const int32_t *env_ids, int num_views,
                      uint8_t *rgb_dev, float *depth_dev, int32_t *seg_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!cam) return fail(TREX_E_INVALID, "trex_batch_render: camera is null");
  if (width <= 0 || height <= 0 || width > TREX_RENDER_MAXDIM || height > TREX_RENDER_MAXDIM)
    return fail(TREX_E_INVALID, "trex_batch_render: width and height must lie in [1, " + std::to_string(TREX_RENDER_MAXDIM) + "]");
  if (!rgb_dev && !depth_dev && !seg_dev) return fail(TREX_E_INVALID, "trex_batch_render: all three outputs are null");
  trex::CameraBasis cb;
  if (int c = built([&] { cb = trex::camera_basis(*cam, width, height); })) return c;
  if (env_ids) {
    if (num_views <= 0) return fail(TREX_E_INVALID, "trex_batch_render: num_views must be positive");
    for (int v = 0; v < num_views; v++)
      if (env_ids[v] < 0 || env_ids[v] >= b->n)
        return fail(TREX_E_INVALID, "trex_batch_render: env id " + std::to_string(env_ids[v]) + " out of range [0, " +
                                        std::to_string(b->n) + ")");
  } else {
    if (num_views != 0 && num_views != b->n) return fail(TREX_E_INVALID, "trex_batch_render: env_ids NULL needs num_views 0 or N");
    num_views = b->n;
  }
  if (num_views > 65535) return fail(TREX_E_INVALID, "trex_batch_render: at most 65535 views per call");
  DeviceGuard guard(b->device);
  const size_t px = (size_t)num_views * height * width;
  BUF_TRY(b, rgb_dev, px * 3, "trex_batch_render: rgb");
  BUF_TRY(b, depth_dev, px * sizeof(float), "trex_batch_render: depth");
  BUF_TRY(b, seg_dev, px * sizeof(int32_t), "trex_batch_render: seg");
  hipStream_t s = (hipStream_t)stream;
  if (int c = ensure_render_table(b, "trex_batch_render")) return c;
  if (env_ids) {
    if (b->render_ids.bytes < (size_t)num_views * sizeof(int32_t)) {   // (grows rarely: the old buffer may still be read by an earlier call)
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(b->render_ids.alloc((size_t)num_views * sizeof(int32_t), false));
    }
    HIP_TRY(hipMemcpyAsync(b->render_ids.p, env_ids, (size_t)num_views * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  TrexRenderArgs a = query_args<TrexRenderArgs>(b);
  a.env_ids = env_ids ? b->render_ids.as<int32_t>() : nullptr;
  a.prim = b->render_prim.as<TrexRenderPrim>(); a.plane = b->render_plane.as<float4>();
  a.rgb = rgb_dev; a.depth = depth_dev; a.seg = seg_dev;
  a.num_views = num_views; a.width = width; a.height = height;
  a.nprim = b->render_nprim; a.follow_base = cam->follow_base != 0;
  for (int c = 0; c < 3; c++) {
    a.target[c] = cam->target[c]; a.offset[c] = cb.offset[c];
    a.fwd[c] = cb.fwd[c]; a.right[c] = cb.right[c]; a.up[c] = cb.up[c];
  }
  a.tan_y = cb.tan_y; a.tan_x = cb.tan_x;
  a.near_z = cam->near_z; a.far_z = cam->far_z;
  a.floor_z = (float)b->floor_z;
  HIP_TRY(trex_launch_render(a, s));
  return TREX_OK;
}

int trex_batch_ray_test(TrexBatch *b, const float *rays_dev, int num_rays, int shared, int link, uint32_t body_mask, int hit_floor,
                        float *fraction_dev, int32_t *body_dev, float *position_dev, float *normal_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!rays_dev || !fraction_dev) return fail(TREX_E_INVALID, "trex_batch_ray_test: rays or fraction is null");
  if (num_rays < 1 || num_rays > TREX_RAY_MAXRAYS)
    return fail(TREX_E_INVALID, "trex_batch_ray_test: num_rays " + std::to_string(num_rays) + " outside [1, " +
                                    std::to_string(TREX_RAY_MAXRAYS) + "]");
  if (int c = check_link(b, "trex_batch_ray_test", link, -1)) return c;
  DeviceGuard guard(b->device);
  const size_t nr = (size_t)b->n * num_rays;
  BUF_TRY(b, rays_dev, (shared ? (size_t)num_rays : nr) * 6 * sizeof(float), "trex_batch_ray_test: rays");
  BUF_TRY(b, fraction_dev, nr * sizeof(float), "trex_batch_ray_test: fraction");
  BUF_TRY(b, body_dev, nr * sizeof(int32_t), "trex_batch_ray_test: body");
  BUF_TRY(b, position_dev, nr * 3 * sizeof(float), "trex_batch_ray_test: position");
  BUF_TRY(b, normal_dev, nr * 3 * sizeof(float), "trex_batch_ray_test: normal");
  if (int c = ensure_render_table(b, "trex_batch_ray_test")) return c;
  TrexRayArgs a = query_args<TrexRayArgs>(b);
  a.rays = rays_dev; a.fraction = fraction_dev; a.body = body_dev; a.position = position_dev; a.normal = normal_dev;
  a.num_rays = num_rays; a.shared = shared != 0;
  a.link_body = -1;
  if (link >= 0) {   // the frame of the link in its body: body <- link of "link_tf"
    a.link_body = b->links.body[link];
    trex::tf12(b->links.tf[link], a.link_tf);
  }
  a.nprim = b->render_nprim; a.hit_floor = hit_floor != 0;
  a.body_mask = b->nb >= 32 ? body_mask : body_mask & ((1u << b->nb) - 1u);   // (bits beyond the model's bodies mean nothing)
  a.floor_z = (float)b->floor_z;
  HIP_TRY(trex_launch_ray_test(a, b->render_prim.as<TrexRenderPrim>(), b->render_plane.as<float4>(), (hipStream_t)stream));
  return TREX_OK;
}

// ---- link kinematics (link_state.hip)
int trex_batch_set_link_probes(TrexBatch *b, int set, const int32_t *link_host, const double *local_xyz_host, int num_probes) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (set < 0 || set >= TREX_LINK_SETS)
    return fail(TREX_E_INVALID, "trex_batch_set_link_probes: set " + std::to_string(set) + " outside [0, " + std::to_string(TREX_LINK_SETS) + ")");
  if (num_probes < 0 || num_probes > TREX_LINK_MAXPROBES)
    return fail(TREX_E_INVALID, "trex_batch_set_link_probes: num_probes " + std::to_string(num_probes) + " outside [0, " +
                                    std::to_string(TREX_LINK_MAXPROBES) + "]");
  if (num_probes > 0 && (!link_host || !local_xyz_host)) return fail(TREX_E_INVALID, "trex_batch_set_link_probes: null argument");
  trex::ProbeTable t;
  if (int c = built([&] { t = trex::build_probe_table(b->links, link_host, local_xyz_host, num_probes); })) return c;
  DeviceGuard guard(b->device);
  DeviceBuf body, tf;
  if (num_probes > 0) {
    HIP_TRY(body.alloc(t.body.size() * sizeof(int32_t), false));
    HIP_TRY(tf.alloc(t.tf.size() * sizeof(float), false));
    HIP_TRY(hipMemcpy(body.p, t.body.data(), body.bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tf.p, t.tf.data(), tf.bytes, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  TrexBatch::ProbeSet &ps = b->probes[set];
  ps.n = num_probes; ps.body = std::move(body); ps.tf = std::move(tf); ps.host_body = std::move(t.body);   // (frees the old table)
  return TREX_OK;
}

int trex_batch_link_state(TrexBatch *b, int set, int axes, int proper, const float *accel_dev, float *pose_dev, float *velocity_dev,
                          float *acceleration_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (int c = check_probe_set(b, "trex_batch_link_state", set)) return c;
  const TrexBatch::ProbeSet &ps = b->probes[set];
  if (axes < TREX_AXES_WORLD || axes > TREX_AXES_BASE)
    return fail(TREX_E_INVALID, "trex_batch_link_state: axes " + std::to_string(axes) + " outside 0..2");
  if (!pose_dev && !velocity_dev && !acceleration_dev) return fail(TREX_E_INVALID, "trex_batch_link_state: all three outputs are null");
  DeviceGuard guard(b->device);
  const size_t nk = (size_t)b->n * ps.n;
  if (acceleration_dev) BUF_TRY(b, accel_dev, (size_t)b->n * (6 + b->nj) * sizeof(float), "trex_batch_link_state: accel");
  BUF_TRY(b, pose_dev, nk * 7 * sizeof(float), "trex_batch_link_state: pose");
  BUF_TRY(b, velocity_dev, nk * 6 * sizeof(float), "trex_batch_link_state: velocity");
  BUF_TRY(b, acceleration_dev, nk * 6 * sizeof(float), "trex_batch_link_state: acceleration");
  TrexLinkArgs a = query_args<TrexLinkArgs>(b);
  a.accel = acceleration_dev ? accel_dev : nullptr;
  a.probe_body = ps.body.as<int32_t>(); a.probe_tf = ps.tf.as<float>();
  a.pose = pose_dev; a.vel = velocity_dev; a.acc = acceleration_dev;
  a.num_probes = ps.n; a.D = 6 + b->nj;
  a.axes = axes; a.proper = proper != 0;
  fill_base(b, a);
  HIP_TRY(trex_launch_link_state(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- inverse kinematics (inverse_kinematics.hip)
int trex_batch_inverse_kinematics(TrexBatch *b, int set, const int32_t *mode_host, int frame, const float *target_dev,
                                  const float *q_init_dev, uint32_t joint_mask, const TrexIkParams *params, float *q_out_dev,
                                  float *info_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_inverse_kinematics: ";
  if (int c = check_probe_set(b, "trex_batch_inverse_kinematics", set)) return c;
  const TrexBatch::ProbeSet &ps = b->probes[set];
  if (ps.n > TREX_IK_MAXPROBES)
    return fail(TREX_E_INVALID, me + "probe set " + std::to_string(set) + " holds " + std::to_string(ps.n) + " probes, at most " +
                                    std::to_string(TREX_IK_MAXPROBES) + " can be targets");
  if (!mode_host || !target_dev || !q_out_dev) return fail(TREX_E_INVALID, me + "null argument");
  if (frame != TREX_AXES_WORLD && frame != TREX_AXES_BASE)
    return fail(TREX_E_INVALID, me + "frame " + std::to_string(frame) + " is neither TREX_AXES_WORLD nor TREX_AXES_BASE");
  if (frame == TREX_AXES_BASE && b->links.body[0] != 0) return fail(TREX_E_INVALID, me + "URDF link 0 does not belong to the base body");
  trex::IkTask t;
  if (int c = built([&] { t = trex::build_ik_task(ps.host_body, b->parent, b->obs_order, mode_host, joint_mask, params); })) return c;
  DeviceGuard guard(b->device);
  const size_t nj = (size_t)b->n * b->nj * sizeof(float);
  BUF_TRY(b, target_dev, (size_t)b->n * ps.n * 7 * sizeof(float), "trex_batch_inverse_kinematics: target");
  BUF_TRY(b, q_init_dev, nj, "trex_batch_inverse_kinematics: q_init");
  BUF_TRY(b, q_out_dev, nj, "trex_batch_inverse_kinematics: q_out");
  BUF_TRY(b, info_dev, (size_t)b->n * 4 * sizeof(float), "trex_batch_inverse_kinematics: info");
  TrexIkArgs a = query_args<TrexIkArgs>(b);
  a.probe_tf = ps.tf.as<float>(); a.target = target_dev; a.q_init = q_init_dev; a.q_out = q_out_dev; a.info = info_dev;
  a.nb = b->nb; a.K = ps.n; a.M = t.rows; a.frame = frame;
  trex::tf12(b->links.tf[0], a.base_tf);   // URDF link 0's frame in the base body
  std::memcpy(a.body, t.body, sizeof a.body); std::memcpy(a.mode, t.mode, sizeof a.mode); std::memcpy(a.row0, t.row0, sizeof a.row0);
  std::memcpy(a.chain, t.chain, sizeof a.chain);
  a.move_mask = t.move_mask;
  a.iterations = t.iterations; a.damping2 = t.damping2; a.gain = t.gain; a.max_step = t.max_step;
  a.tol_pos = t.tol_pos; a.tol_ori = t.tol_ori;
  HIP_TRY(trex_launch_inverse_kinematics(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- proximity queries (proximity.hip)
int trex_batch_set_proximity_shapes(TrexBatch *b, const int32_t *body_host, const double *capsule_host, int num_capsules,
                                    const int32_t *pair_host, int num_pairs) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::ProxTable t;
  if (int c = built([&] { t = trex::build_prox_table(b->nb, body_host, capsule_host, num_capsules, pair_host, num_pairs); })) return c;
  DeviceGuard guard(b->device);
  DeviceBuf blob;
  if (t.caps > 0) {
    HIP_TRY(blob.alloc(t.blob.size(), false));
    HIP_TRY(hipMemcpy(blob.p, t.blob.data(), blob.bytes, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  t.blob = {};
  b->prox.blob = std::move(blob);   // (frees the old table)
  b->prox.table = std::move(t);
  return TREX_OK;
}

int trex_batch_proximity(TrexBatch *b, float *distance_dev, float *point_a_dev, float *point_b_dev, float *normal_dev,
                         int32_t *capsule_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const trex::ProxTable &pt = b->prox.table;
  if (pt.caps < 1) return fail(TREX_E_INVALID, "trex_batch_proximity: no table is set (trex_batch_set_proximity_shapes)");
  if (!distance_dev) return fail(TREX_E_INVALID, "trex_batch_proximity: distance is null");
  DeviceGuard guard(b->device);
  const size_t np = (size_t)b->n * pt.pairs;
  BUF_TRY(b, distance_dev, np * sizeof(float), "trex_batch_proximity: distance");
  BUF_TRY(b, point_a_dev, np * 3 * sizeof(float), "trex_batch_proximity: point_a");
  BUF_TRY(b, point_b_dev, np * 3 * sizeof(float), "trex_batch_proximity: point_b");
  BUF_TRY(b, normal_dev, np * 3 * sizeof(float), "trex_batch_proximity: normal");
  BUF_TRY(b, capsule_dev, np * 2 * sizeof(int32_t), "trex_batch_proximity: capsule");
  TrexProxArgs a = query_args<TrexProxArgs>(b);
  const char *blob = b->prox.blob.as<char>();
  a.cap = (const float *)blob; a.cap_body = (const int32_t *)(blob + pt.o_body);
  a.test = (const uint32_t *)(blob + pt.o_test); a.pair_first = (const int32_t *)(blob + pt.o_first);
  a.distance = distance_dev; a.point_a = point_a_dev; a.point_b = point_b_dev; a.normal = normal_dev; a.capsule = capsule_dev;
  a.num_capsules = pt.caps; a.num_pairs = pt.pairs; a.num_tests = pt.tests;
  HIP_TRY(trex_launch_proximity(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- observation channels (observation.hip)
int trex_batch_set_observation(TrexBatch *b, const TrexObsChannel *channels_host, int num_channels, int *extra_dim_out) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::ObsTable t;
  if (int c = built([&] { t = trex::build_obs_table(b->links, b->nj, b->action_cols(), channels_host, num_channels); })) return c;
  DeviceGuard guard(b->device);
  DeviceBuf blob;
  if (t.channels > 0) {
    HIP_TRY(blob.alloc(t.blob.size(), false));
    HIP_TRY(hipMemcpy(blob.p, t.blob.data(), blob.bytes, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  t.blob = {};
  if (extra_dim_out) *extra_dim_out = t.extra;
  b->observation.blob = std::move(blob);   // (frees the old table)
  b->observation.table = std::move(t);
  return TREX_OK;
}

int trex_batch_observation_dim(const TrexBatch *b) {
  if (check_batch(b)) return TREX_E_INVALID;
  return 3 * b->nj + b->observation.table.extra;
}

int trex_batch_compose_rows(TrexBatch *b, const float *rows_dev, int row_stride, const float *actions_dev, const float *extern_dev,
                            int extern_stride, float *out_rows_dev, int out_stride, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_compose_rows: ";
  const trex::ObsTable &ot = b->observation.table;
  if (ot.channels < 1) return fail(TREX_E_INVALID, me + "no channels are set (trex_batch_set_observation)");
  if (!rows_dev || !out_rows_dev) return fail(TREX_E_INVALID, me + "rows or out_rows is null");
  const int nobs = 3 * b->nj, tail = b->pen_in_rows ? 5 : 2, width = nobs + ot.extra + tail;
  if (row_stride < nobs + tail) return fail(TREX_E_INVALID, me + "row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  if (out_stride < width) return fail(TREX_E_INVALID, me + "out_stride " + std::to_string(out_stride) + " < " + std::to_string(width) +
                                                          " = 3J + E + the tail");
  if (ot.contact && !b->sens_on) return fail(TREX_E_INVALID, me + "a CONTACT_FORCE channel is set and the contact sensor is off (trex_batch_set_contact_sensor)");
  if (ot.actions && ot.action_cols != b->action_cols())
    return fail(TREX_E_INVALID, me + "the action rows are " + std::to_string(b->action_cols()) + " wide, the PREV_ACTION channel was set with " +
                                    std::to_string(ot.action_cols) + " (set the channels again)");
  if (ot.extern_cols > 0) {
    if (!extern_dev) return fail(TREX_E_INVALID, me + "an EXTERNAL channel is set and extern is null");
    if (extern_stride < ot.extern_cols)
      return fail(TREX_E_INVALID, me + "extern_stride " + std::to_string(extern_stride) + " < " + std::to_string(ot.extern_cols) +
                                      ", the columns of the EXTERNAL channels");
  }
  const size_t n = (size_t)b->n;
  const size_t rows_bytes = trex::row_block_bytes(n, row_stride, nobs + tail), out_bytes = trex::row_block_bytes(n, out_stride, width);
  if (trex::ranges_overlap(rows_dev, rows_bytes, out_rows_dev, out_bytes)) return fail(TREX_E_INVALID, me + "out_rows overlaps rows");
  DeviceGuard guard(b->device);
  BUF_TRY(b, rows_dev, rows_bytes, "trex_batch_compose_rows: rows");
  BUF_TRY(b, out_rows_dev, out_bytes, "trex_batch_compose_rows: out_rows");
  if (ot.actions) BUF_TRY(b, actions_dev, n * ot.action_cols * sizeof(float), "trex_batch_compose_rows: actions");
  if (ot.extern_cols > 0) BUF_TRY(b, extern_dev, trex::row_block_bytes(n, extern_stride, ot.extern_cols), "trex_batch_compose_rows: extern");
  TrexObsArgs a = query_args<TrexObsArgs>(b);
  const char *blob = b->observation.blob.as<char>();
  a.chan = (const TrexObsChan *)blob; a.col_chan = (const uint8_t *)(blob + ot.o_col);
  a.rows = rows_dev; a.actions = ot.actions ? actions_dev : nullptr; a.ext = ot.extern_cols > 0 ? extern_dev : nullptr;
  a.sens = ot.contact ? b->sens.as<float>() : nullptr;
  a.out = out_rows_dev;
  a.D = 6 + b->nj; a.nobs = nobs; a.extra = ot.extra; a.tail = tail;
  a.row_stride = row_stride; a.out_stride = out_stride; a.ext_stride = extern_stride; a.act_cols = ot.action_cols;
  a.body_mask = ot.body_mask | fill_base(b, a);
  HIP_TRY(trex_launch_observation(a, (hipStream_t)stream));
  return TREX_OK;
}

// ---- reward terms (reward.hip)
int trex_batch_set_reward(TrexBatch *b, const TrexRewardTerm *terms_host, int num_terms) {
  if (check_batch(b)) return TREX_E_INVALID;
  trex::RewTable t;
  trex::RewardHistLayout l;
  if (int c = built([&] {
        t = trex::build_reward_table(b->links, b->obs_order, b->nb, b->action_cols(), terms_host, num_terms);
        l = trex::reward_hist_layout(b->n, t.action_cols, b->nj, t.terms);
      }))
    return c;
  DeviceGuard guard(b->device);
  DeviceBuf blob, hist;
  if (t.terms > 0) {
    HIP_TRY(blob.alloc(t.blob.size(), false));
    HIP_TRY(hipMemcpy(blob.p, t.blob.data(), blob.bytes, hipMemcpyHostToDevice));
    HIP_TRY(hist.alloc(l.bytes, true));
  }
  HIP_TRY(hipDeviceSynchronize());   // (no launch still reads the table this one replaces; the new one is in place on every stream)
  t.blob = {};
  TrexBatch::Reward &r = b->reward;
  r.blob = std::move(blob);   // (frees the old table and its history)
  r.hist = std::move(hist);
  r.table = std::move(t);
  r.st = {};
  if (r.hist)
    r.st = {member_at<float>(r.hist, l.prev_act), member_at<float>(r.hist, l.prev_qd), member_at<float>(r.hist, l.timer),
            member_at<float>(r.hist, l.held), member_at<int32_t>(r.hist, l.valid)};
  return TREX_OK;
}

int trex_batch_reward_terms(const TrexBatch *b) {
  if (check_batch(b)) return TREX_E_INVALID;
  return b->reward.table.terms;
}

int trex_batch_compose_reward(TrexBatch *b, float *rows_dev, int row_stride, const float *actions_dev, const float *command_dev,
                              float *terms_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const std::string me = "trex_batch_compose_reward: ";
  const TrexBatch::Reward &r = b->reward;
  const trex::RewTable &rt = r.table;
  if (rt.terms < 1) return fail(TREX_E_INVALID, me + "no terms are set (trex_batch_set_reward)");
  if (!rows_dev) return fail(TREX_E_INVALID, me + "rows is null");
  const int nobs = 3 * b->nj, tail = b->pen_in_rows ? 5 : 2;
  if (row_stride < nobs + tail) return fail(TREX_E_INVALID, me + "row_stride < 3J + 2 (3J + 5 with penalties in rows)");
  if (rt.contact && !b->sens_on) return fail(TREX_E_INVALID, me + "a contact term is set and the contact sensor is off (trex_batch_set_contact_sensor)");
  if (rt.command && !command_dev) return fail(TREX_E_INVALID, me + "a tracking term is set and command is null");
  if (rt.actions && !actions_dev) return fail(TREX_E_INVALID, me + "ACTION_RATE is set and actions is null");
  if (rt.actions && rt.action_cols != b->action_cols())
    return fail(TREX_E_INVALID, me + "the action rows are " + std::to_string(b->action_cols()) + " wide, ACTION_RATE was set with " +
                                    std::to_string(rt.action_cols) + " (set the terms again)");
  const size_t n = (size_t)b->n;
  DeviceGuard guard(b->device);
  BUF_TRY(b, rows_dev, trex::row_block_bytes(n, row_stride, nobs + tail), "trex_batch_compose_reward: rows");
  if (rt.actions) BUF_TRY(b, actions_dev, n * rt.action_cols * sizeof(float), "trex_batch_compose_reward: actions");
  if (rt.command) BUF_TRY(b, command_dev, n * 3 * sizeof(float), "trex_batch_compose_reward: command");
  BUF_TRY(b, terms_dev, n * rt.terms * sizeof(float), "trex_batch_compose_reward: terms");
  TrexRewArgs a = query_args<TrexRewArgs>(b);
  const char *blob = r.blob.as<char>();
  a.term = (const TrexRewTerm *)blob; a.joint_body = (const int32_t *)(blob + rt.o_joint);
  a.rows = rows_dev; a.actions = rt.actions ? actions_dev : nullptr; a.command = rt.command ? command_dev : nullptr;
  a.sens = rt.contact ? b->sens.as<float>() : nullptr;
  a.terms_out = terms_dev;
  a.prev_act = r.st.prev_act; a.prev_qd = r.st.prev_qd; a.timer = r.st.timer; a.held = r.st.held; a.valid = r.st.valid;
  a.D = 6 + b->nj; a.nj = b->nj; a.num_terms = rt.terms; a.row_stride = row_stride; a.act_cols = rt.action_cols;
  a.Ts = (float)b->step_seconds;
  a.body_mask = rt.body_mask | fill_base(b, a);
  HIP_TRY(trex_launch_reward(a, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_reward_reset(TrexBatch *b, const uint8_t *mask_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Reward &r = b->reward;
  if (r.table.terms < 1) return fail(TREX_E_INVALID, "trex_batch_reward_reset: no terms are set (trex_batch_set_reward)");
  DeviceGuard guard(b->device);
  BUF_TRY(b, mask_dev, (size_t)b->n, "trex_batch_reward_reset: mask");
  HIP_TRY(trex_launch_reward_reset(mask_dev, b->n, r.table.terms, r.st.timer, r.st.held, r.st.valid, (hipStream_t)stream));
  return TREX_OK;
}

// ---- floor clearance and fall termination (termination.hip)
int trex_batch_body_clearance(TrexBatch *b, float *clearance_dev, float *lowest_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  if (!clearance_dev) return fail(TREX_E_INVALID, "trex_batch_body_clearance: clearance is null");
  DeviceGuard guard(b->device);
  const size_t nb = (size_t)b->n * b->nb;
  BUF_TRY(b, clearance_dev, nb * sizeof(float), "trex_batch_body_clearance: clearance");
  BUF_TRY(b, lowest_dev, nb * 3 * sizeof(float), "trex_batch_body_clearance: lowest");
  TrexTermArgs t = query_args<TrexTermArgs>(b);
  t.hull = b->arr.hull;
  t.clearance = clearance_dev; t.lowest = lowest_dev;
  HIP_TRY(trex_launch_termination(t, 0, (hipStream_t)stream));
  return TREX_OK;
}

int trex_batch_termination_info(TrexBatch *b, int32_t *reason_dev, float *values_dev, float *terminal_obs_dev, void *stream) {
  if (check_batch(b)) return TREX_E_INVALID;
  const TrexBatch::Termination &tm = b->term;
  if (!tm.blob) return fail(TREX_E_INVALID, "trex_batch_termination_info: termination was never enabled (trex_batch_set_termination)");
  DeviceGuard guard(b->device);
  const size_t n = (size_t)b->n;
  BUF_TRY(b, reason_dev, n * sizeof(int32_t), "trex_batch_termination_info: reason");
  BUF_TRY(b, values_dev, n * 3 * sizeof(float), "trex_batch_termination_info: values");
  BUF_TRY(b, terminal_obs_dev, n * 3 * b->nj * sizeof(float), "trex_batch_termination_info: terminal_obs");
  hipStream_t s = (hipStream_t)stream;
  if (reason_dev) HIP_TRY(hipMemcpyAsync(reason_dev, tm.reason, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (values_dev) HIP_TRY(hipMemcpyAsync(values_dev, tm.values, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (terminal_obs_dev) HIP_TRY(hipMemcpyAsync(terminal_obs_dev, tm.tobs, n * 3 * b->nj * sizeof(float), hipMemcpyDeviceToDevice, s));
  return TREX_OK;
}

}  // extern "C"
