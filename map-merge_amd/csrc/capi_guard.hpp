// capi_guard.hpp -- how an extern "C" entry point of libmm3d.so (include/mm3d.h) runs its work: under the context's lock, on
// its device, every exception turned into a status and the context's error text.  capi.cpp holds nearly all entry points; a
// test hook whose work lives in one kernel file (fpfh.hip::mm3d_debug_pair_bins) has its entry point there, so that the
// library's host code links without that file (tests/host_san).
#pragma once

#include <exception>
#include <mutex>
#include <new>

#include "types.hpp"

namespace mm3d {

template <class F>
int guarded(mm3d_ctx *ctx, F &&f)
{
  if (!ctx) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  // error flags waiting for the next sync() belong to the call that recorded them: a call that ends with an
  // exception must not leave them (their pinned words get reused) to the next one, on this context or its helpers
  struct Clean {
    mm3d_ctx *c;
    ~Clean()
    {
      auto one = [](mm3d_ctx *r) {
        r->deferred.clear();
        r->private_objects = false;
        for (mm3d_ctx *h : r->helpers) { h->deferred.clear(); h->private_objects = false; }
      };
      one(c);
      for (mm3d_ctx *p : c->peers) one(p);
    }
  } clean{ctx};
  try {
    if (hipSetDevice(ctx->device) != hipSuccess) throw Error(MM3D_EDEVICE, "hipSetDevice failed");
    f();
    if (!ctx->deferred.empty()) ctx->sync();      // nothing recorded by this call is left unchecked
    return MM3D_OK;
  } catch (const Error &e) {
    ctx->err = e.what();
    return e.status;
  } catch (const std::bad_alloc &) {
    ctx->err = "out of host memory";
    return MM3D_ENOMEM;
  } catch (const std::exception &e) {
    ctx->err = e.what();
    return MM3D_EDEVICE;
  } catch (...) {
    ctx->err = "unknown error";
    return MM3D_EDEVICE;
  }
}

}  // namespace mm3d
