// libm_debug.hip -- test hook: evaluates the restated glibc functions (libm_exact.hpp) and the other device primitives the
// bit-equal claims rest on, so the tests can hold the device's results against the host's argument by argument
// (tests/test_libm_exact.py).
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

}  // namespace mm3d
