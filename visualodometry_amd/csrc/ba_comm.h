// The sharded BA's communicator (ba_comm.hip): an RCCL communicator, or an in-process loopback
// group standing in for one.  RCCL's own header stays in ba_comm.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>

struct vo_ctx;
typedef struct ncclComm* ncclComm_t;  // as rccl.h declares it

namespace vo {

struct LoopGroup;  // vo_comm_init_loopback's group (ba_comm.hip)

struct Comm {
  ncclComm_t comm = nullptr;
  std::shared_ptr<LoopGroup> loop;
  int nranks = 1, rank = 0;
  ~Comm();
  // in-place all-reduce of n elements (int32 min or float64 sum) on the context stream
  template <class T>
  void allreduce(T* dbuf, size_t n, bool is_min, hipStream_t st);  // T: int32_t, double
};

// entry points used by api.hip
void comm_unique_id(char out[128]);
void comm_init(vo_ctx* ctx, int nranks, int rank, const char id[128]);
void comm_init_loopback(vo_ctx* ctx, int nranks, int rank, const char id[128]);

}  // namespace vo
