// wxengine: RCCL bound at run time, for the lat-band transport (wx_band_rccl_init / wx_band_step_rccl).
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is bound with dlopen when a communicator is requested

#include <string>

#include "wx_spec.h"   // StateError

namespace wx {

// RCCL bound at run time (no link dependency: single-GPU users never load it).  In a torch process the already-loaded
// librccl is found first, so the engine and torch.distributed share one RCCL.
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  static RcclApi& get() {
    static RcclApi api;
    if (api.lib) return api;
    for (const char* name : {"librccl.so", "librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
      if (api.lib) break;
    }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) {
      if (api.lib) break;
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!api.lib) throw StateError(std::string("RCCL not found (librccl.so): ") + dlerror());
    auto sym = [&](const char* n) {
      void* p = dlsym(api.lib, n);
      if (!p) throw StateError(std::string("RCCL symbol missing: ") + n);
      return p;
    };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    return api;
  }
  void check(ncclResult_t r, const char* what) const {
    if (r != ncclSuccess) throw StateError(std::string("RCCL ") + what + ": " + GetErrorString(r));
  }
};

}  // namespace wx
