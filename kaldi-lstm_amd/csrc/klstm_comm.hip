// kaldi-lstm_amd/csrc/klstm_comm.hip -- the communicator entries of include/klstm.h (klstm_comm_*, klstm_allreduce_buffer) over RCCL.
// The engine's gradient all-reduce (klstm_engine.hip klstm_allreduce_grads) goes through klstm_allreduce_buffer.
#include <cstring>
#include <mutex>
#include <string>

#include <dlfcn.h>
#include <rccl/rccl.h>          // types only: the library is resolved at run time (below)

#include "klstm_host.h"

using namespace klstm;

// ---- RCCL (data-parallel training over utterance streams: ONE sum-all-reduce of the gradient blob per minibatch) ----
// libklstm.so has no link-time dependency on RCCL: the entry points are looked up in the process when the first DP call
// arrives -- first among the symbols already loaded (a host framework may have brought its own librccl, e.g. PyTorch's
// bundled one; two copies of RCCL in one process must not be mixed), then by dlopen("librccl.so.1").
namespace {
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
  std::string why;
};
RcclApi &rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    void *h = nullptr;
    auto sym = [&](const char *name) -> void * {
      void *p = dlsym(RTLD_DEFAULT, name);
      if (!p) {
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) p = dlsym(h, name);
      }
      return p;
    };
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.CommCount = reinterpret_cast<decltype(api.CommCount)>(sym("ncclCommCount"));
    api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(sym("ncclAllReduce"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce;
    if (!api.ok) api.why = std::string("RCCL entry points not found (") + (dlerror() ? dlerror() : "librccl.so.1 not loadable") + ")";
  });
  return api;
}
klstm_status rccl_fail(const char *what, ncclResult_t r) {
  RcclApi &a = rccl();
  return fail(KLSTM_ERR_HIP, "%s failed: %s", what, a.GetErrorString ? a.GetErrorString(r) : "RCCL error");
}
}  // namespace
extern "C" {

klstm_status klstm_comm_get_unique_id(void *id128) {
  if (!id128) return fail(KLSTM_ERR_ARG, "klstm_comm_get_unique_id: null argument");
  RcclApi &a = rccl();
  if (!a.ok) return fail(KLSTM_ERR_HIP, "%s", a.why.c_str());
  ncclUniqueId id;
  const ncclResult_t r = a.GetUniqueId(&id);
  if (r != ncclSuccess) return rccl_fail("ncclGetUniqueId", r);
  static_assert(sizeof(id) == KLSTM_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(id128, &id, sizeof(id));
  return KLSTM_OK;
}
klstm_status klstm_comm_init_rank(int device, int nranks, int rank, const void *id128, void **comm) {
  if (!id128 || !comm || nranks <= 0 || rank < 0 || rank >= nranks) return fail(KLSTM_ERR_ARG, "klstm_comm_init_rank: bad argument");
  RcclApi &a = rccl();
  if (!a.ok) return fail(KLSTM_ERR_HIP, "%s", a.why.c_str());
  HIPCHK(hipSetDevice(device));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t c = nullptr;
  const ncclResult_t r = a.CommInitRank(&c, nranks, id, rank);
  if (r != ncclSuccess) return rccl_fail("ncclCommInitRank", r);
  *comm = c;
  return KLSTM_OK;
}
klstm_status klstm_comm_destroy(void *comm) {
  if (!comm) return KLSTM_OK;
  RcclApi &a = rccl();
  if (!a.ok) return fail(KLSTM_ERR_HIP, "%s", a.why.c_str());
  const ncclResult_t r = a.CommDestroy(static_cast<ncclComm_t>(comm));
  return r == ncclSuccess ? KLSTM_OK : rccl_fail("ncclCommDestroy", r);
}
klstm_status klstm_comm_count(void *comm, int *nranks) {
  if (!comm || !nranks) return fail(KLSTM_ERR_ARG, "klstm_comm_count: null argument");
  RcclApi &a = rccl();
  if (!a.ok || !a.CommCount) return fail(KLSTM_ERR_HIP, "%s", a.ok ? "ncclCommCount not found" : a.why.c_str());
  const ncclResult_t r = a.CommCount(static_cast<ncclComm_t>(comm), nranks);
  return r == ncclSuccess ? KLSTM_OK : rccl_fail("ncclCommCount", r);
}
klstm_status klstm_allreduce_buffer(float *buf_dev, size_t n, void *rccl_comm, void *hip_stream) {
  if (!buf_dev || !rccl_comm) return fail(KLSTM_ERR_ARG, "klstm_allreduce_buffer: null argument");
  if (n == 0) return KLSTM_OK;
  RcclApi &a = rccl();
  if (!a.ok) return fail(KLSTM_ERR_HIP, "%s", a.why.c_str());
  const ncclResult_t r = a.AllReduce(buf_dev, buf_dev, n, ncclFloat32, ncclSum, static_cast<ncclComm_t>(rccl_comm),
                                     static_cast<hipStream_t>(hip_stream));
  return r == ncclSuccess ? KLSTM_OK : rccl_fail("ncclAllReduce", r);
}

}  // extern "C"
