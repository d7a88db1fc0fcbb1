// capi.cpp -- the extern "C" boundary of libmm3d.so (include/mm3d.h).  Nothing throws across it.
#include <algorithm>
#include <cstdlib>
#include <sstream>
#include <string>

#include "device_util.hpp"
#include "capi_guard.hpp"
#include "drivers.hpp"

using namespace mm3d;

namespace {

const char *kDescNames[] = {"PFH", "PFHRGB", "FPFH", "RSD", "SHOT", "SC3D"};
const char *kDescFields[] = {"pfh", "pfhrgb", "fpfh", "r_min", "shot", "shape_context"};
const int kDescDims[] = {125, 250, 33, 2, 1344, 1980};
const char *kKpNames[] = {"SIFT", "HARRIS"};
const char *kEstNames[] = {"MATCHING", "SAC_IA"};

int from_string(const char *s, const char *const *names, int n)
{
  if (!s) return MM3D_EINVAL;
  for (int i = 0; i < n; ++i)
    if (std::string(names[i]) == s) return i;
  return MM3D_EINVAL;
}

}  // namespace

mm3d::StageSelection::StageSelection()
{
  mm3d_alignment_options_default(&align_options);
  mm3d_keypoint_options_default(&keypoint_options);
  mm3d_refine_options_default(&refine_options);
  mm3d_coarse_options_default(&coarse_options);
  mm3d_confidence_options_default(&confidence_options);
  mm3d_icp_rejection_options_default(&reject_options);
  mm3d_icp_robust_options_default(&robust_options);
  mm3d_icp_color_options_default(&color_options);
  mm3d_icp_generalized_options_default(&generalized_options);
  mm3d_estimator_options_default(&estimator_options);
  mm3d_icp_sampling_options_default(&sampling_options);
  mm3d_outlier_options_default(&outlier_options);
  mm3d_cluster_options_default(&cluster_options);
  mm3d_smooth_options_default(&smooth_options);
  mm3d_plane_options_default(&plane_options);
  mm3d_icp_geometry_options_default(&geometry_options);
}

extern "C" {

// ---------------------------------------------------------------- enums / params
const char *mm3d_descriptor_name(int d) { return (d >= 0 && d < 6) ? kDescNames[d] : nullptr; }
int mm3d_descriptor_from_string(const char *s) { return from_string(s, kDescNames, 6); }
const char *mm3d_descriptor_field_name(int d) { return (d >= 0 && d < 6) ? kDescFields[d] : nullptr; }
int mm3d_descriptor_dim(int d) { return (d >= 0 && d < 6) ? kDescDims[d] : MM3D_EINVAL; }
const char *mm3d_keypoint_name(int k) { return (k >= 0 && k < 2) ? kKpNames[k] : nullptr; }
int mm3d_keypoint_from_string(const char *s) { return from_string(s, kKpNames, 2); }
const char *mm3d_estimation_method_name(int m) { return (m >= 0 && m < 2) ? kEstNames[m] : nullptr; }
int mm3d_estimation_method_from_string(const char *s) { return from_string(s, kEstNames, 2); }

void mm3d_params_default(mm3d_params *p)
{
  if (!p) return;
  p->resolution = 0.1;
  p->descriptor_radius = p->resolution * 8.0;
  p->outliers_min_neighbours = 50;
  p->normal_radius = p->resolution * 6.0;
  p->keypoint_type = MM3D_KP_SIFT;
  p->keypoint_threshold = 5.0;
  p->descriptor_type = MM3D_DESC_PFH;
  p->estimation_method = MM3D_EST_MATCHING;
  p->refine_transform = 1;
  p->inlier_threshold = p->resolution * 5.0;
  p->max_correspondence_distance = p->inlier_threshold * 2.0;
  p->max_iterations = 500;
  p->matching_k = 5;
  p->transform_epsilon = 1e-2;
  p->confidence_threshold = 0.0;
  p->output_resolution = 0.05;
}

// pcl::console::parse_argument semantics: the first occurrence of "--name" (argv[1..]) followed by a
// value is taken; unknown options are ignored; a bool is atoi(value) == 1.
int mm3d_params_from_command_line(int argc, const char *const *argv, mm3d_params *p)
{
  if (!p || (argc > 0 && !argv)) return MM3D_EINVAL;
  mm3d_params_default(p);
  auto find = [&](const char *name) -> const char * {
    for (int i = 1; i < argc; ++i)   // pcl::console::find_argument
      if (argv[i] && std::string(argv[i]) == name) return (i + 1 < argc) ? argv[i + 1] : nullptr;
    return nullptr;
  };
  auto get_d = [&](const char *name, double &v) { if (const char *s = find(name)) v = std::atof(s); };
  auto get_i = [&](const char *name, int &v) { if (const char *s = find(name)) v = std::atoi(s); };
  get_d("--resolution", p->resolution);
  get_d("--descriptor_radius", p->descriptor_radius);
  get_i("--outliers_min_neighbours", p->outliers_min_neighbours);
  get_d("--normal_radius", p->normal_radius);
  if (const char *s = find("--keypoint_type"); s && *s) {
    int v = mm3d_keypoint_from_string(s);
    if (v < 0) return MM3D_EINVAL;
    p->keypoint_type = v;
  }
  get_d("--keypoint_threshold", p->keypoint_threshold);
  if (const char *s = find("--descriptor_type"); s && *s) {
    int v = mm3d_descriptor_from_string(s);
    if (v < 0) return MM3D_EINVAL;
    p->descriptor_type = v;
  }
  if (const char *s = find("--estimation_method"); s && *s) {
    int v = mm3d_estimation_method_from_string(s);
    if (v < 0) return MM3D_EINVAL;
    p->estimation_method = v;
  }
  if (const char *s = find("--refine_transform")) p->refine_transform = std::atoi(s) == 1;   // parse_argument(bool&)
  get_d("--inlier_threshold", p->inlier_threshold);
  get_d("--max_correspondence_distance", p->max_correspondence_distance);
  get_i("--max_iterations", p->max_iterations);
  int matching_k = -1;
  get_i("--matching_k", matching_k);
  if (matching_k > 0) p->matching_k = (uint64_t)matching_k;
  get_d("--transform_epsilon", p->transform_epsilon);
  get_d("--confidence_threshold", p->confidence_threshold);
  get_d("--output_resolution", p->output_resolution);
  return MM3D_OK;
}

size_t mm3d_params_to_string(const mm3d_params *p, char *buf, size_t cap)
{
  if (!p) return 0;
  std::ostringstream s;
  s << "resolution: " << p->resolution << std::endl;
  s << "descriptor_radius: " << p->descriptor_radius << std::endl;
  s << "outliers_min_neighbours: " << p->outliers_min_neighbours << std::endl;
  s << "normal_radius: " << p->normal_radius << std::endl;
  s << "keypoint_type: " << (mm3d_keypoint_name(p->keypoint_type) ? mm3d_keypoint_name(p->keypoint_type) : "?") << std::endl;
  s << "keypoint_threshold: " << p->keypoint_threshold << std::endl;
  s << "descriptor_type: " << (mm3d_descriptor_name(p->descriptor_type) ? mm3d_descriptor_name(p->descriptor_type) : "?") << std::endl;
  s << "estimation_method: "
    << (mm3d_estimation_method_name(p->estimation_method) ? mm3d_estimation_method_name(p->estimation_method) : "?") << std::endl;
  s << "refine_transform: " << (p->refine_transform ? 1 : 0) << std::endl;
  s << "inlier_threshold: " << p->inlier_threshold << std::endl;
  s << "max_correspondence_distance: " << p->max_correspondence_distance << std::endl;
  s << "max_iterations: " << p->max_iterations << std::endl;
  s << "matching_k: " << p->matching_k << std::endl;
  s << "transform_epsilon: " << p->transform_epsilon << std::endl;
  s << "confidence_threshold: " << p->confidence_threshold << std::endl;
  s << "output_resolution: " << p->output_resolution << std::endl;
  const std::string str = s.str();
  if (buf && cap) {
    size_t m = std::min(cap - 1, str.size());
    std::memcpy(buf, str.data(), m);
    buf[m] = 0;
  }
  return str.size() + 1;
}

// ---------------------------------------------------------------- the opt-in stages' options and their record
void mm3d_alignment_options_default(mm3d_alignment_options *o)
{
  if (o) *o = mm3d_alignment_options{MM3D_ALIGN_SAC_IA, 1 << 16, 10, 0.9, 0.25};
}
void mm3d_keypoint_options_default(mm3d_keypoint_options *o)
{
  if (o) *o = mm3d_keypoint_options{MM3D_KEYPOINTS_REFERENCE, 0.0};
}
void mm3d_refine_options_default(mm3d_refine_options *o)
{
  if (o) *o = mm3d_refine_options{MM3D_REFINE_ICP, 0.0, 7, 6, 0.01};
}
void mm3d_coarse_options_default(mm3d_coarse_options *o)
{
  if (o) *o = mm3d_coarse_options{MM3D_COARSE_NONE, 0.0, 4, 720, 6, 32, 0.5, 0.9, 3, 0.25};
}
void mm3d_confidence_options_default(mm3d_confidence_options *o)
{
  if (o) *o = mm3d_confidence_options{MM3D_CONFIDENCE_REFERENCE, 0.0, 8, 0.05, 0};
}
void mm3d_icp_rejection_options_default(mm3d_icp_rejection_options *o)
{
  if (o) *o = mm3d_icp_rejection_options{0, MM3D_REJECT_NONE, 0.5, 0, 1.0};
}
void mm3d_icp_geometry_options_default(mm3d_icp_geometry_options *o)
{
  if (o) *o = mm3d_icp_geometry_options{0, 0.0, 90.0, 3, 0, 45.0};
}

void mm3d_icp_robust_options_default(mm3d_icp_robust_options *o)
{
  if (o) *o = mm3d_icp_robust_options{MM3D_ROBUST_OFF, 0.05, 0.0, 0.5, 0.0};
}
void mm3d_icp_color_options_default(mm3d_icp_color_options *o)
{
  if (o) *o = mm3d_icp_color_options{0, 0.968, 0.0, 4};
}
void mm3d_icp_generalized_options_default(mm3d_icp_generalized_options *o)
{
  if (o) *o = mm3d_icp_generalized_options{0, 1e-3};
}
void mm3d_estimator_options_default(mm3d_estimator_options *o)
{
  if (o) *o = mm3d_estimator_options{MM3D_ESTIMATOR_RANSAC, 0.0, 64, 20};
}
void mm3d_outlier_options_default(mm3d_outlier_options *o)
{
  if (o) *o = mm3d_outlier_options{MM3D_OUTLIERS_RADIUS, 16, 2.0};
}
void mm3d_cluster_options_default(mm3d_cluster_options *o)
{
  if (o) *o = mm3d_cluster_options{MM3D_CLUSTERS_OFF, 100, 0.0};
}
void mm3d_plane_options_default(mm3d_plane_options *o)
{
  if (o) *o = mm3d_plane_options{MM3D_PLANES_OFF, 1, 1024, 1, 1u, 0.0, 0.05, {0.0, 0.0, 1.0}, 10.0};
}
void mm3d_smooth_options_default(mm3d_smooth_options *o)
{
  if (o) *o = mm3d_smooth_options{MM3D_SMOOTH_OFF, 2, 6, MM3D_SMOOTH_MAPS | MM3D_SMOOTH_COMPOSED, 0.0};
}

void mm3d_icp_sampling_options_default(mm3d_icp_sampling_options *o)
{
  if (o) *o = mm3d_icp_sampling_options{MM3D_ICP_SAMPLE_NONE, 0.25, 0, 4};
}

// ---------------------------------------------------------------- context
static std::string &create_error()
{
  static thread_local std::string e = "null context";
  return e;
}

int mm3d_create(int device, mm3d_ctx **out)
{
  if (!out) return MM3D_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
    create_error() = "mm3d_create: no HIP device " + std::to_string(device) + " (" + std::to_string(count) + " visible)";
    return MM3D_EDEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) { create_error() = "mm3d_create: hipSetDevice failed"; return MM3D_EDEVICE; }
  auto *c = new (std::nothrow) mm3d_ctx();
  if (!c) return MM3D_ENOMEM;
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return MM3D_EDEVICE; }
  *out = c;
  return MM3D_OK;
}

// One process, several GPUs (the reference's caller is one process: R/src/map_merge_node.cpp:133-153).  The context is the
// first device's; the others' root contexts hang off it (mm3d_ctx::peers), and a DeviceSet holds the RCCL communicators.
int mm3d_create_devices(const int *devices, int n_devices, mm3d_ctx **out)
{
  if (!out) return MM3D_EINVAL;
  *out = nullptr;
  if (!devices || n_devices < 1 || n_devices > 64) return MM3D_EINVAL;
  mm3d_ctx *root = nullptr;
  int st = mm3d_create(devices[0], &root);
  if (st != MM3D_OK) return st;
  for (int d = 1; d < n_devices && st == MM3D_OK; ++d) {
    mm3d_ctx *p = nullptr;
    st = mm3d_create(devices[d], &p);
    if (st == MM3D_OK) root->peers.push_back(p);
  }
  if (st == MM3D_OK) {
    try {
      root->device_set = device_set_create(devices, n_devices);
    } catch (const Error &e) {
      st = e.status;
      create_error() = e.what();
    } catch (...) {
      st = MM3D_EDEVICE;
      create_error() = "mm3d_create_devices: unknown failure";
    }
  }
  if (st != MM3D_OK) { mm3d_destroy(root); return st; }
  (void)hipSetDevice(devices[0]);
  *out = root;
  return MM3D_OK;
}

int mm3d_device_count(const mm3d_ctx *ctx) { return ctx ? (int)ctx->peers.size() + 1 : 0; }
int mm3d_device_at(const mm3d_ctx *ctx, int i)
{
  if (!ctx || i < 0 || i > (int)ctx->peers.size()) return MM3D_EINVAL;
  return i == 0 ? ctx->device : ctx->peers[(size_t)i - 1]->device;
}
int mm3d_devices_use_rccl(const mm3d_ctx *ctx) { return ctx && device_set_has_comms(ctx->device_set) ? 1 : 0; }

static void set_streams_one(mm3d_ctx *ctx, int n_streams)
{
  if (hipSetDevice(ctx->device) != hipSuccess) throw Error(MM3D_EDEVICE, "hipSetDevice failed");
  while ((int)ctx->helpers.size() + 1 > n_streams) {
    mm3d_destroy(ctx->helpers.back());
    ctx->helpers.pop_back();
  }
  while ((int)ctx->helpers.size() + 1 < n_streams) {
    mm3d_ctx *h = nullptr;
    const int st = mm3d_create(ctx->device, &h);
    if (st != MM3D_OK) throw Error(st, "mm3d_set_streams: could not create a helper context");
    h->sel = ctx->sel;                                  // (whatever was selected before mm3d_set_streams)
    ctx->helpers.push_back(h);
  }
}

int mm3d_set_streams(mm3d_ctx *ctx, int n_streams)
{
  if (n_streams < 1 || n_streams > 64) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    set_streams_one(ctx, n_streams);
    for (mm3d_ctx *p : ctx->peers) set_streams_one(p, n_streams);     // (every device of an mm3d_create_devices context)
    (void)hipSetDevice(ctx->device);
  });
}

int mm3d_get_streams(const mm3d_ctx *ctx) { return ctx ? (int)ctx->helpers.size() + 1 : 0; }

void mm3d_destroy(mm3d_ctx *ctx)
{
  if (!ctx) return;
  device_set_destroy(ctx->device_set);                  // (the communicators go before the streams they were used on)
  ctx->device_set = nullptr;
  delete ctx->map_cache;                                // (its buffers go back to the pools of the contexts that made them)
  ctx->map_cache = nullptr;
  for (mm3d_ctx *p : ctx->peers) mm3d_destroy(p);
  ctx->peers.clear();
  for (mm3d_ctx *h : ctx->helpers) mm3d_destroy(h);
  ctx->helpers.clear();
  (void)hipSetDevice(ctx->device);
  (void)stream_wait(ctx->stream);
  for (auto &p : ctx->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  ctx->pool->trim();
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->scan_status) (void)hipFree(ctx->scan_status);
  if (ctx->scan_ticket) (void)hipFree(ctx->scan_ticket);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

// (a null context: why the calling thread's last mm3d_create / mm3d_create_devices failed -- there is no context to ask then)
const char *mm3d_last_error(const mm3d_ctx *ctx) { return ctx ? ctx->err.c_str() : create_error().c_str(); }
int mm3d_last_icp_iterations(const mm3d_ctx *ctx) { return ctx ? ctx->last_icp_iterations : 0; }
int mm3d_last_icp_converged(const mm3d_ctx *ctx) { return ctx ? ctx->last_icp_converged : 0; }
int mm3d_last_run_stage_seconds(const mm3d_ctx *ctx, double *features_s, double *total_s)
{
  if (!ctx) return MM3D_EINVAL;
  if (features_s) *features_s = ctx->last_features_s;
  if (total_s) *total_s = ctx->last_total_s;
  return MM3D_OK;
}
int mm3d_last_run_device_seconds(const mm3d_ctx *ctx, double *exchange_s, double *pairs_s, double *gather_s)
{
  if (!ctx) return MM3D_EINVAL;
  if (exchange_s) *exchange_s = ctx->last_exchange_s;
  if (pairs_s) *pairs_s = ctx->last_pairs_s;
  if (gather_s) *gather_s = ctx->last_gather_s;
  return MM3D_OK;
}
size_t mm3d_last_run_map_sizes(const mm3d_ctx *ctx, size_t *points, size_t *keypoints, size_t capacity)
{
  if (!ctx) return 0;
  const size_t n = ctx->last_points.size();
  for (size_t i = 0; i < n && i < capacity; ++i) {
    if (points) points[i] = ctx->last_points[i];
    if (keypoints) keypoints[i] = ctx->last_keypoints[i];
  }
  return n;
}
void mm3d_set_debug(mm3d_ctx *ctx, int on)
{
  if (!ctx) return;
  ctx->debug = on != 0;
  ctx->knn_fallback_rows = ctx->knn_rows = 0;
  ctx->knn_paths = 0;
}
unsigned mm3d_debug_knn_paths(mm3d_ctx *ctx)
{
  if (!ctx) return 0;
  const unsigned m = ctx->knn_paths;
  ctx->knn_paths = 0;
  return m;
}
long long mm3d_debug_knn_fallback_rows(mm3d_ctx *ctx) { return ctx ? ctx->knn_fallback_rows : 0; }
long long mm3d_debug_knn_rows(mm3d_ctx *ctx) { return ctx ? ctx->knn_rows : 0; }
void mm3d_debug_waits(mm3d_ctx *ctx, long long out[2])
{
  out[0] = ctx ? ctx->waits : 0;
  out[1] = ctx ? ctx->wait_ns : 0;
  if (ctx) {                      // (with the worker contexts of mm3d_set_streams, on every device: the whole library call's waits)
    for (mm3d_ctx *h : ctx->helpers) { out[0] += h->waits; out[1] += h->wait_ns; }
    for (mm3d_ctx *p : ctx->peers) {
      out[0] += p->waits; out[1] += p->wait_ns;
      for (mm3d_ctx *h : p->helpers) { out[0] += h->waits; out[1] += h->wait_ns; }
    }
  }
}
int mm3d_debug_float_chain(mm3d_ctx *ctx, const float *incr, const unsigned *hits, int n, float *out)
{
  if (n < 0 || (n && (!incr || !hits || !out))) return MM3D_EINVAL;
  return guarded(ctx, [&] { debug_float_chain(ctx, incr, hits, n, out); });
}
int mm3d_debug_libm(mm3d_ctx *ctx, int fn, const float *x, const float *y, int n, float *out)
{
  const bool two = fn == 4 || fn == 7 || fn == 8 || fn == 9;
  if (n < 0 || fn < 0 || fn > 11 || (n && (!x || !out || (two && !y)))) return MM3D_EINVAL;
  return guarded(ctx, [&] { debug_libm(ctx, fn, x, y, n, out); });
}
// (mm3d_debug_pair_bins: csrc/fpfh.hip)
int mm3d_debug_sift_cert_octave(mm3d_ctx *ctx, const mm3d_cloud *points, double min_scale, int octave, float *val, float *bound, size_t capacity,
                                size_t *n_out)
{
  if (!points || !n_out || octave < 0 || (capacity && (!val || !bound))) return MM3D_EINVAL;
  return guarded(ctx, [&] { *n_out = debug_sift_cert_octave(ctx, points, min_scale, octave, val, bound, capacity); });
}
void mm3d_debug_sift_cert_stats(long long out[8], int reset) { if (out) debug_sift_cert_stats(out, reset); }
void mm3d_debug_sift_cert_min(int n) { debug_sift_cert_min(n); }
float mm3d_debug_cloud_voxel_leaf(const mm3d_cloud *cloud) { return cloud ? cloud->voxel_leaf : 0.0f; }
void mm3d_debug_sacia_stats(long long out[4], int reset, int collect) { if (out) debug_sacia_stats(out, reset, collect); }
void mm3d_srand(mm3d_ctx *ctx, unsigned seed) { if (ctx) ctx->rnd.seed(seed); }
int mm3d_synchronize(mm3d_ctx *ctx) { return guarded(ctx, [&] { ctx->sync(); }); }

// ---------------------------------------------------------------- objects
int mm3d_cloud_create(mm3d_ctx *ctx, const void *points, size_t n, size_t stride, size_t rgba_offset, mm3d_cloud **out)
{
  if (!out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = cloud_from_memory(ctx, points, n, stride, rgba_offset); ctx->sync(); });
}
size_t mm3d_cloud_size(const mm3d_cloud *c) { return c ? c->n : 0; }
int mm3d_cloud_download(mm3d_ctx *ctx, const mm3d_cloud *c, void *dst, size_t stride, size_t rgba_offset)
{
  if (!c || (!dst && c->n)) return MM3D_EINVAL;
  return guarded(ctx, [&] { cloud_download(ctx, c, dst, stride, rgba_offset); });
}
void mm3d_cloud_free(mm3d_ctx *ctx, mm3d_cloud *c)
{
  if (!ctx || !c) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  (void)stream_wait(ctx->stream);
  delete c;
}

size_t mm3d_normals_size(const mm3d_normals *n) { return n ? n->n : 0; }
int mm3d_normals_download(mm3d_ctx *ctx, const mm3d_normals *n, void *dst, size_t stride)
{
  if (!n || (!dst && n->n) || stride < 16 || stride % 4) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    if (!n->n) return;
    MM3D_HIP(hipMemcpy2DAsync(dst, stride, n->nrm.get(), 16, 16, n->n, hipMemcpyDefault, ctx->stream));
    ctx->sync();
  });
}
int mm3d_normals_create(mm3d_ctx *ctx, const void *normals, size_t n, size_t stride, mm3d_normals **out)
{
  if (!out || stride < 16 || stride % 4 || (!normals && n)) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    auto *r = new mm3d_normals();
    r->n = n;
    r->nrm = DevBuf<float4>(ctx, n);
    if (n) {
      MM3D_HIP(hipMemcpy2DAsync(r->nrm.get(), 16, normals, stride, 16, n, hipMemcpyDefault, ctx->stream));
      ctx->sync();
    }
    *out = r;
  });
}
void mm3d_normals_free(mm3d_ctx *ctx, mm3d_normals *n)
{
  if (!ctx || !n) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  (void)stream_wait(ctx->stream);
  delete n;
}

size_t mm3d_desc_size(const mm3d_desc *d) { return d ? d->n : 0; }
int mm3d_desc_dim(const mm3d_desc *d) { return d ? d->dim : 0; }
int mm3d_desc_type(const mm3d_desc *d) { return d ? d->type : MM3D_EINVAL; }
int mm3d_desc_download(mm3d_ctx *ctx, const mm3d_desc *d, float *dst)
{
  if (!d || (!dst && d->n)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    if (!d->n) return;
    MM3D_HIP(hipMemcpyAsync(dst, d->data.get(), d->n * d->dim * sizeof(float), hipMemcpyDefault, ctx->stream));
    ctx->sync();
  });
}
int mm3d_desc_download_frames(mm3d_ctx *ctx, const mm3d_desc *d, float *dst)
{
  if (!d || (!dst && d->n)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    if (d->type != MM3D_DESC_SHOT || (d->n && !d->rf.get())) throw Error(MM3D_EINVAL, "these descriptors carry no reference frames");
    if (!d->n) return;
    MM3D_HIP(hipMemcpyAsync(dst, d->rf.get(), d->n * 9 * sizeof(float), hipMemcpyDefault, ctx->stream));
    ctx->sync();
  });
}

int mm3d_debug_desc_knn(mm3d_ctx *ctx, const float *a, size_t na, const float *b, size_t nb, int dim, int k, int *idx, float *d2)
{
  if (!a || !b || !idx || !d2 || na == 0 || nb == 0 || dim < 1 || k < 1) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    auto make = [&](const float *data, size_t n) {
      std::unique_ptr<mm3d_desc> r(new mm3d_desc());
      r->n = n; r->dim = dim; r->type = -1;
      r->data = DevBuf<float>(ctx, n * (size_t)dim);
      MM3D_HIP(hipMemcpyAsync(r->data.get(), data, n * (size_t)dim * sizeof(float), hipMemcpyDefault, ctx->stream));
      return r;
    };
    std::unique_ptr<mm3d_desc> A = make(a, na), B = make(b, nb);
    DevBuf<int> di;
    DevBuf<float> dd;
    desc_knn(ctx, A.get(), B.get(), k, di, dd);
    MM3D_HIP(hipMemcpyAsync(idx, di.get(), na * (size_t)k * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MM3D_HIP(hipMemcpyAsync(d2, dd.get(), na * (size_t)k * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}

int mm3d_desc_create(mm3d_ctx *ctx, const float *data, size_t n, int descriptor_type, mm3d_desc **out)
{
  if (!out || (!data && n)) return MM3D_EINVAL;
  *out = nullptr;
  if (mm3d_descriptor_dim(descriptor_type) < 0) return MM3D_EINVAL;
  return guarded(ctx, [&] { *out = desc_from_memory(ctx, data, n, descriptor_type); });
}
void mm3d_desc_free(mm3d_ctx *ctx, mm3d_desc *d)
{
  if (!ctx || !d) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  (void)stream_wait(ctx->stream);
  delete d;
}

// ---------------------------------------------------------------- features.h
int mm3d_downsample(mm3d_ctx *ctx, const mm3d_cloud *in, double resolution, mm3d_cloud **out)
{
  if (!in || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = downsample(ctx, in, resolution); });
}

int mm3d_remove_outliers(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, int min_neighbours, mm3d_cloud **out)
{
  if (!in || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = remove_outliers(ctx, in, radius, min_neighbours); });
}

int mm3d_compute_normals(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, mm3d_normals **out)
{
  if (!in || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = compute_normals(ctx, in, radius); ctx->sync(); });
}

int mm3d_detect_keypoints(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, int type, double threshold,
                          double radius, double resolution, mm3d_cloud **keypoints)
{
  (void)normals; (void)radius;
  if (!points || !keypoints) return MM3D_EINVAL;
  *keypoints = nullptr;
  return guarded(ctx, [&] {
    if (type == MM3D_KP_SIFT) {
      // detectKeypointsSIFT(points, resolution, 3, 3, threshold)  (features.cpp:92)
      *keypoints = detect_keypoints_sift(ctx, points, resolution, 3, 3, threshold);
    } else if (type == MM3D_KP_HARRIS) {
      // detectKeypointsHarris(points, normals, threshold, radius)  (features.cpp:94)
      if (!normals) throw Error(MM3D_EINVAL, "HARRIS keypoints need the surface normals");
      *keypoints = detect_keypoints_harris(ctx, points, normals, threshold, radius);
    } else {
      throw Error(MM3D_EINVAL, "invalid keypoint type");
    }
  });
}

int mm3d_harris_response(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, double radius, float *dst)
{
  if (!points || !normals || (!dst && points->n)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    DevBuf<float> r;
    harris_response(ctx, points, normals, radius, r);
    if (points->n) MM3D_HIP(hipMemcpyAsync(dst, r.get(), points->n * sizeof(float), hipMemcpyDefault, ctx->stream));
    ctx->sync();
  });
}

int mm3d_compute_descriptors(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, mm3d_cloud *keypoints,
                             int descriptor, double feature_radius, mm3d_desc **out)
{
  if (!points || !normals || !keypoints || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    if (descriptor == MM3D_DESC_FPFH) {
      *out = compute_fpfh(ctx, points, normals, keypoints, feature_radius);
    } else if (descriptor == MM3D_DESC_PFH) {
      *out = compute_pfh(ctx, points, normals, keypoints, feature_radius);
    } else if (descriptor == MM3D_DESC_PFHRGB) {
      *out = compute_pfhrgb(ctx, points, normals, keypoints, feature_radius);
    } else if (descriptor == MM3D_DESC_RSD) {
      *out = compute_rsd(ctx, points, normals, keypoints, feature_radius);
    } else if (descriptor == MM3D_DESC_SHOT) {
      *out = compute_shot(ctx, points, normals, keypoints, feature_radius);
    } else if (descriptor == MM3D_DESC_SC3D) {
      *out = compute_sc3d(ctx, points, normals, keypoints, feature_radius);
    } else {
      throw Error(MM3D_EINVAL, "unknown descriptor type");   // dispatch_descriptors.h:63
    }
  });
}

// ---------------------------------------------------------------- matching.h
int mm3d_find_correspondences(mm3d_ctx *ctx, const mm3d_desc *source, const mm3d_desc *target, size_t k, mm3d_corr *out,
                              size_t cap, size_t *n)
{
  if (!source || !target || !n) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    // assertDescriptorsPair / dispatch by field name: both sides must be the same descriptor kind
    if (source->type != target->type) throw Error(MM3D_EINVAL, "descriptor types differ");
    std::vector<mm3d_corr> v;
    find_correspondences(ctx, source, target, k, v);
    *n = v.size();
    if (out) {
      if (cap < v.size()) throw Error(MM3D_ECAPACITY, "correspondence buffer too small");
      std::memcpy(out, v.data(), v.size() * sizeof(mm3d_corr));
    }
  });
}

int mm3d_estimate_transform_from_correspondences(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_cloud *tkp,
                                                 const mm3d_corr *corr, size_t n_corr, double inlier_threshold, float T[16],
                                                 mm3d_corr *inliers, size_t cap, size_t *n_inliers)
{
  if (!skp || !tkp || (!corr && n_corr) || !T) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    std::vector<mm3d_corr> inl;
    ransac_transform(ctx, skp, tkp, corr, n_corr, inlier_threshold, T, inl);
    if (n_inliers) *n_inliers = inl.size();
    if (inliers) {
      if (cap < inl.size()) throw Error(MM3D_ECAPACITY, "inlier buffer too small");
      std::memcpy(inliers, inl.data(), inl.size() * sizeof(mm3d_corr));
    }
  });
}

int mm3d_estimate_transform_from_descriptors(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp,
                                             const mm3d_desc *td, double min_sample_distance, double max_corr_dist,
                                             int max_iterations, float T[16])
{
  if (!skp || !sd || !tkp || !td || !T) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    if (sd->type != td->type) throw Error(MM3D_EINVAL, "descriptor types differ");
    sac_ia(ctx, skp, sd, tkp, td, min_sample_distance, max_corr_dist, max_iterations, T, true);
  });
}

int mm3d_estimate_transform_icp(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float guess[16],
                                double max_corr_dist, double outlier_rejection_threshold, int max_iterations, double eps,
                                float T[16])
{
  (void)outlier_rejection_threshold;   // setRANSACOutlierRejectionThreshold: no rejector is registered in the reference
  if (!source || !target || !guess || !T) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    IcpResult r = icp(ctx, source, target, guess, max_corr_dist, max_iterations, eps);
    std::memcpy(T, r.T, sizeof(r.T));
  });
}

int mm3d_estimate_transform(mm3d_ctx *ctx, const mm3d_cloud *sp, const mm3d_cloud *skp, const mm3d_desc *sd,
                            const mm3d_cloud *tp, const mm3d_cloud *tkp, const mm3d_desc *td, int method, int refine,
                            double inlier_threshold, double max_corr_dist, int max_iterations, size_t matching_k, double eps,
                            float T[16])
{
  if (!sp || !skp || !sd || !tp || !tkp || !td || !T) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    estimate_transform(ctx, sp, skp, sd, tp, tkp, td, method, refine, inlier_threshold, max_corr_dist, max_iterations,
                       matching_k, eps, T, true);
  });
}

int mm3d_transform_score(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                         double max_distance, double *score)
{
  if (!source || !target || !T || !score) return MM3D_EINVAL;
  return guarded(ctx, [&] { *score = transform_score(ctx, source, target, T, max_distance); });
}

// ---------------------------------------------------------------- map bundles
int mm3d_map_features(mm3d_ctx *ctx, const mm3d_cloud *raw, const mm3d_params *params, mm3d_map **out)
{
  if (!raw || !params || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = map_features_impl(ctx, raw, params).release(); });
}

const mm3d_cloud *mm3d_map_points(const mm3d_map *m) { return m ? m->points : nullptr; }
const mm3d_cloud *mm3d_map_keypoints(const mm3d_map *m) { return m ? m->keypoints : nullptr; }
const mm3d_desc *mm3d_map_descriptors(const mm3d_map *m) { return m ? m->desc : nullptr; }

int mm3d_map_from_parts(mm3d_ctx *ctx, mm3d_cloud *points, mm3d_cloud *keypoints, mm3d_desc *desc, mm3d_map **out)
{
  if (!ctx || !points || !keypoints || !desc || !out) return MM3D_EINVAL;
  if (keypoints->n != desc->n) return MM3D_EINVAL;
  *out = make_map(std::unique_ptr<mm3d_cloud>(points), std::unique_ptr<mm3d_cloud>(keypoints), std::unique_ptr<mm3d_desc>(desc)).release();
  return MM3D_OK;
}

int mm3d_map_prepare(mm3d_ctx *ctx, mm3d_map *m, const mm3d_params *p)
{
  if (!m || !p) return MM3D_EINVAL;
  return guarded(ctx, [&] { map_prepare_impl(ctx, m, p); });
}

void mm3d_map_free(mm3d_ctx *ctx, mm3d_map *m)
{
  if (!ctx || !m) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  (void)stream_wait(ctx->stream);
  delete m;
}

int mm3d_pair_estimate(mm3d_ctx *ctx, const mm3d_map *source, const mm3d_map *target, const mm3d_params *params, int execute,
                       mm3d_pair_result *out)
{
  if (!source || !target || !params || !out) return MM3D_EINVAL;
  return guarded(ctx, [&] { pair_estimate_impl(ctx, source, target, params, execute != 0, out); });
}

int mm3d_pairs_skip(mm3d_ctx *ctx, const mm3d_map *const *sources, const mm3d_map *const *targets, size_t n, const mm3d_params *params)
{
  if (!params || (n && (!sources || !targets))) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    for (size_t i = 0; i < n; ++i) {
      const mm3d_map *s = sources[i], *t = targets[i];
      if (!s || !t) throw Error(MM3D_EINVAL, "null map");
      if (is_pair(s, t)) pair_replay_draws(ctx->rnd, ctx, params, cloud_host(ctx, s->keypoints));
    }
  });
}

int mm3d_global_transforms(const mm3d_pair_result *pairs, size_t n_pairs, double confidence_threshold, size_t n_clouds,
                           float *out_T, size_t *n_out)
{
  if ((!pairs && n_pairs) || !out_T || !n_out) return MM3D_EINVAL;
  try {
    return global_transforms(pairs, n_pairs, confidence_threshold, n_clouds, out_T, n_out);
  } catch (...) {
    return MM3D_ENOMEM;
  }
}

// ---------------------------------------------------------------- map_merging.h
int mm3d_estimate_maps_transforms(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params,
                                  float *out_T, size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out)
{
  if (!params || !n_out || (n && (!clouds || !out_T))) return MM3D_EINVAL;
  if (n_pairs_out) *n_pairs_out = 0;
  *n_out = 0;
  if (n == 0) return MM3D_OK;                       // {} -> {}  (map_merging.cpp:192-194)
  if (n == 1) {                                     // one cloud -> {Identity}, the cloud is not touched (:195-197)
    std::memset(out_T, 0, sizeof(float) * 16);
    out_T[0] = out_T[5] = out_T[10] = out_T[15] = 1.0f;
    *n_out = 1;
    return MM3D_OK;
  }
  return guarded(ctx, [&] {
    if (ctx->device_set) {                             // a device list (mm3d_create_devices), even of one device
      estimate_maps_devices(ctx, clouds, n, params, out_T, n_out, pairs_out, n_pairs_out);
      return;
    }
    // mm3d_set_map_cache: what this call adds is committed only when it succeeds (a throw below aborts it)
    struct CacheCall {
      MapCacheBase *c;
      bool ok = false;
      ~CacheCall() { if (c && !ok) c->abort(); }
    } cache_call{ctx->map_cache};
    if (ctx->map_cache) ctx->map_cache->begin(n, params, ctx->sel);
    if (!ctx->helpers.empty())
      estimate_maps_streams(ctx, clouds, n, params, out_T, n_out, pairs_out, n_pairs_out);
    else
      estimate_maps_sequential(ctx, clouds, n, params, out_T, n_out, pairs_out, n_pairs_out);
    if (ctx->map_cache) ctx->map_cache->commit();
    cache_call.ok = true;
  });
}

int mm3d_compose_maps(mm3d_ctx *ctx, const mm3d_cloud *const *clouds, size_t n, const float *transforms, size_t n_transforms,
                      double resolution, mm3d_cloud **out)
{
  if (!out) return MM3D_EINVAL;
  *out = nullptr;
  if (n == 0) return MM3D_OK;                       // nullptr (map_merging.cpp:281-283)
  if (n != n_transforms) {                          // the reference throws (map_merging.cpp:285-288)
    if (ctx) ctx->err = "composeMaps: clouds and transforms size must be the same.";
    return MM3D_EINVAL;
  }
  if (!clouds || !transforms) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    std::unique_ptr<mm3d_cloud> cat(transform_concat(ctx, clouds, n, transforms));
    *out = downsample(ctx, cat.get(), resolution);
    // (mm3d_set_smoothing with MM3D_SMOOTH_COMPOSED: the layers that the pairs' residuals left side by side are fused between two
    // voxel passes -- the first bounds the density the kernel sees, the last makes one point per voxel of what came together)
    if (ctx->sel.smoother && (ctx->sel.smooth_options.where & MM3D_SMOOTH_COMPOSED)) {
      std::unique_ptr<mm3d_cloud> first(*out);
      *out = nullptr;
      std::unique_ptr<mm3d_cloud> smooth(ctx->sel.smoother->smooth(ctx, first.get(), ctx->sel.smooth_options, resolution, &ctx->last_smooth_stats));
      first.reset();
      *out = downsample(ctx, smooth.get(), resolution);
    }
  });
}

// ---------------------------------------------------------------- measurement
int mm3d_profile_enable(mm3d_ctx *ctx, int on)
{
  return guarded(ctx, [&] {
    ctx->prof_resolve();
    ctx->prof_on = on != 0;
    for (mm3d_ctx *h : ctx->helpers) { h->prof_resolve(); h->prof_on = on != 0; }   // mm3d_set_streams helpers
    for (mm3d_ctx *p : ctx->peers) {                                                // mm3d_create_devices: the other devices
      (void)hipSetDevice(p->device);
      p->prof_resolve();
      p->prof_on = on != 0;
      for (mm3d_ctx *h : p->helpers) { h->prof_resolve(); h->prof_on = on != 0; }
    }
    (void)hipSetDevice(ctx->device);
  });
}
void mm3d_profile_reset(mm3d_ctx *ctx)
{
  if (!ctx) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  auto reset_one = [](mm3d_ctx *r) {
    (void)hipSetDevice(r->device);
    try { r->prof_resolve(); } catch (...) {}
    for (auto &e : r->prof) e = ProfEntry();
    for (mm3d_ctx *h : r->helpers) {
      try { h->prof_resolve(); } catch (...) {}
      for (auto &e : h->prof) e = ProfEntry();
    }
  };
  reset_one(ctx);
  for (mm3d_ctx *p : ctx->peers) reset_one(p);
  (void)hipSetDevice(ctx->device);
}
int mm3d_profile_count(mm3d_ctx *ctx)
{
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lock(ctx->mu);
  try { ctx->prof_resolve(); } catch (...) {}
  // fold what the helper streams (and, for a device list, the other devices' contexts) recorded into this context's
  // table (summed over streams and devices)
  auto fold = [&](mm3d_ctx *h) {
    (void)hipSetDevice(h->device);
    try { h->prof_resolve(); } catch (...) {}
    for (size_t i = 0; i < h->prof.size(); ++i) {
      const int s = ctx->prof_slot(h->prof_names[i].c_str());
      ctx->prof[s].ms += h->prof[i].ms;
      ctx->prof[s].launches += h->prof[i].launches;
      ctx->prof[s].bytes += h->prof[i].bytes;
      h->prof[i] = ProfEntry();
    }
  };
  for (mm3d_ctx *h : ctx->helpers) fold(h);
  for (mm3d_ctx *p : ctx->peers) {
    fold(p);
    for (mm3d_ctx *h : p->helpers) fold(h);
  }
  (void)hipSetDevice(ctx->device);
  return (int)ctx->prof.size();
}
int mm3d_profile_entry(mm3d_ctx *ctx, int i, const char **name, double *total_ms, uint64_t *launches, double *bytes)
{
  if (!ctx) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (i < 0 || i >= (int)ctx->prof.size()) return MM3D_EINVAL;
  if (name) *name = ctx->prof_names[i].c_str();
  if (total_ms) *total_ms = ctx->prof[i].ms;
  if (launches) *launches = ctx->prof[i].launches;
  if (bytes) *bytes = ctx->prof[i].bytes;
  return MM3D_OK;
}

}  // extern "C"
