// libm_debug.hip -- test hook: evaluates the restated glibc functions (libm_exact.hpp) and the other device primitives the
// bit-equal claims rest on, so the tests can hold the device's results against the host's argument by argument
// (tests/test_libm_exact.py); and every wave reduction / scan of device_util.hpp next to the shuffle loop it replaced
// (tests/test_gpu_wave_primitives.py).
#include "capi_guard.hpp"
#include "device_util.hpp"

namespace mm3d {

// (fn 9, atan2_fast, lives with its only caller in fpfh.hip: debug_atan2_fast)
__global__ void k_debug_libm(int fn, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ rcp, int n,
                             float *__restrict__ out)
{
  // fn 6: the 2^(i/32) table staged in LDS as the SIFT kernels stage it (sift.hip::k_sift_dog_lds); every lane reaches the
  // barrier, the work is guarded instead
  __shared__ uint64_t s_tab[32];
  if (threadIdx.x < 32) lm::exp2f_tab_copy(s_tab, threadIdx.x);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float r;
    switch (fn) {
      case 0: r = lm::expf_glibc(x[i]); break;
      case 1: r = lm::atanf_glibc(x[i]); break;
      case 2: r = lm::sinf_glibc(x[i]); break;
      case 3: r = lm::cosf_glibc(x[i]); break;
      case 5: r = __builtin_amdgcn_exp2f(x[i]); break;       // v_exp_f32 as the certified SIFT pass uses it (sift_cert.hpp)
      case 6: r = lm::expf_glibc_t<false>(x[i], [&](unsigned k) { return s_tab[k]; }); break;
      case 7: r = lm::fdiv_const(x[i], y[i], rcp[i]); break;
      case 8: r = acos_abs_greater(x[i], y[i]) ? 1.0f : 0.0f; break;
      case 10: r = __builtin_amdgcn_rsqf(x[i]); break;
      case 11: r = __builtin_amdgcn_rcpf(x[i]); break;
      default: r = lm::atan2f_glibc(y[i], x[i]); break;
    }
    out[i] = r;
  }
}

void debug_libm(Context *c, int fn, const float *x_host, const float *y_host, int n, float *out_host)
{
  if (n <= 0) return;
  DevBuf<float> x(c, n), y(c, n), o(c, n), rcp(c, fn == 7 ? n : 1);
  MM3D_HIP(hipMemcpyAsync(x.get(), x_host, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (y_host) MM3D_HIP(hipMemcpyAsync(y.get(), y_host, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  std::vector<float> r;
  if (fn == 7) {
    // the reciprocal exactly as sift.hip prepares SiftScales::rcp
    r.resize(n);
    for (int i = 0; i < n; ++i) r[i] = (float)(1.0 / (double)y_host[i]);
    MM3D_HIP(hipMemcpyAsync(rcp.get(), r.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  }
  if (fn == 9)
    debug_atan2_fast(c, x.get(), y.get(), n, o.get());
  else
    MM3D_LAUNCH(c, "debug_libm", 0, k_debug_libm, dim3(div_up(n, 256)), dim3(256), 0, fn, (const float *)x.get(), (const float *)y.get(),
                (const float *)rcp.get(), n, o.get());
  MM3D_HIP(hipMemcpyAsync(out_host, o.get(), (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  c->sync();
}

// ---- the wave primitives against their predecessors ----------------------------------------------------------------
// The shuffle loops device_util.hpp, nn_core.hpp and the kernels' open-coded scans and key minima held until the DPP /
// permlane versions replaced them; kept here, and only here, as what the new ones are measured against.
template <class T>
__device__ __forceinline__ T shfl_sum(T v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}
__device__ __forceinline__ int shfl_min_int(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ int shfl_max_int(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float shfl_min_f(float v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float shfl_max_f(float v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ int shfl_scan_incl(int v, int lane)
{
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ unsigned long long shfl_min_u64(unsigned long long v)
{
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_xor(v, s, kWave);
    v = o < v ? o : v;
  }
  return v;
}

// op: 0 wave_sum(double), 1 wave_sum(float), 2 wave_sum(int), 3 wave_min_int, 4 wave_max_int, 5 wave_min_f, 6 wave_max_f,
// 7 wave_scan_incl, 8 wave_min_u64.  Every lane stores what it holds (whole blocks only: all 64 lanes of every wave are here).
template <class T>
__global__ void __launch_bounds__(256) k_debug_wave(int op, const T *__restrict__ in, T *__restrict__ out_new, T *__restrict__ out_old)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const T v = in[i];
  T a = v, b = v;
  if constexpr (std::is_same_v<T, double>) {
    a = wave_sum(v); b = shfl_sum(v);
  } else if constexpr (std::is_same_v<T, float>) {
    if (op == 1) { a = wave_sum(v); b = shfl_sum(v); }
    else if (op == 5) { a = wave_min_f(v); b = shfl_min_f(v); }
    else { a = wave_max_f(v); b = shfl_max_f(v); }
  } else if constexpr (std::is_same_v<T, int>) {
    if (op == 2) { a = wave_sum(v); b = shfl_sum(v); }
    else if (op == 3) { a = wave_min_int(v); b = shfl_min_int(v); }
    else if (op == 4) { a = wave_max_int(v); b = shfl_max_int(v); }
    else { a = wave_scan_incl(v); b = shfl_scan_incl(v, lane); }
  } else {
    a = wave_min_u64(v); b = shfl_min_u64(v);
  }
  out_new[i] = a;
  out_old[i] = b;
}

template <class T>
static void debug_wave_typed(Context *c, int op, const void *in_host, int n, void *new_host, void *old_host)
{
  DevBuf<T> in(c, n), a(c, n), b(c, n);
  MM3D_HIP(hipMemcpyAsync(in.get(), in_host, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream));
  MM3D_LAUNCH(c, "debug_wave", 0, k_debug_wave<T>, dim3(n / 256), dim3(256), 0, op, (const T *)in.get(), a.get(), b.get());
  MM3D_HIP(hipMemcpyAsync(new_host, a.get(), (size_t)n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(old_host, b.get(), (size_t)n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  c->sync();
}

static void debug_wave_primitives(Context *c, int op, const void *in_host, int n, void *new_host, void *old_host)
{
  if (op == 0) debug_wave_typed<double>(c, op, in_host, n, new_host, old_host);
  else if (op == 1 || op == 5 || op == 6) debug_wave_typed<float>(c, op, in_host, n, new_host, old_host);
  else if (op == 8) debug_wave_typed<unsigned long long>(c, op, in_host, n, new_host, old_host);
  else debug_wave_typed<int>(c, op, in_host, n, new_host, old_host);
}

}  // namespace mm3d

// (the entry point lives with its kernel, like nn.hip's mm3d_debug_nn_search: the host-only builds link capi.cpp without this file)
extern "C" int mm3d_debug_wave_primitives(mm3d_ctx *ctx, int op, const void *in, int n, void *out_new, void *out_old)
{
  if (op < 0 || op > 8 || n <= 0 || n % 256 != 0 || !in || !out_new || !out_old) return MM3D_EINVAL;
  return mm3d::guarded(ctx, [&] { mm3d::debug_wave_primitives(ctx, op, in, n, out_new, out_old); });
}
