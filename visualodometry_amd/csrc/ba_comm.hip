// The sharded BA's communicator: RCCL ranks, or an in-process loopback group (ba_comm.h).
#include "ba_comm.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "vo_ctx.h"

namespace vo {

#define VO_NCCL_CHECK(expr)                                                        \
  do {                                                                               \
    ncclResult_t r_ = (expr);                                                        \
    if (r_ != ncclSuccess) {                                                         \
      ::vo::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr,             \
                      ncclGetErrorString(r_));                                       \
      throw ::vo::Error{VO_ERR_RCCL};                                                \
    }                                                                                \
  } while (0)

// In-process loopback group (vo_comm_init_loopback): N contexts of one process, each
// driven by its own host thread, stand in for N RCCL ranks so that the sharded BA path
// can be tested on one device.  Each all-reduce copies to the host, meets the others at
// a barrier and reduces in rank order (every member computes the identical result).
struct LoopGroup {
  int nranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::vector<char>> slot;
  int arrived = 0;
  long gen = 0;
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const long g = gen;
    if (++arrived == nranks) {
      arrived = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
};

Comm::~Comm() {
  if (comm) ncclCommDestroy(comm);
}

template <class T>
void Comm::allreduce(T* dbuf, size_t n, bool is_min, hipStream_t st) {
  if (!loop) {
    const ncclDataType_t ty = std::is_same<T, double>::value ? ncclFloat64 : ncclInt32;
    VO_NCCL_CHECK(ncclAllReduce(dbuf, dbuf, n, ty, is_min ? ncclMin : ncclSum, comm, st));
    return;
  }
  LoopGroup& G = *loop;
  std::vector<T> mine(n);
  VO_HIP_CHECK(hipMemcpyAsync(mine.data(), dbuf, n * sizeof(T), hipMemcpyDeviceToHost, st));
  VO_HIP_CHECK(hipStreamSynchronize(st));
  {
    std::lock_guard<std::mutex> lk(G.mu);
    G.slot[rank].assign(reinterpret_cast<const char*>(mine.data()),
                        reinterpret_cast<const char*>(mine.data()) + n * sizeof(T));
  }
  G.barrier();
  std::vector<T> out(n);
  for (int r = 0; r < nranks; ++r) {
    const T* v = reinterpret_cast<const T*>(G.slot[r].data());
    for (size_t i = 0; i < n; ++i)
      out[i] = r == 0 ? v[i] : is_min ? std::min(out[i], v[i]) : out[i] + v[i];
  }
  G.barrier();  // every member has read every slot
  VO_HIP_CHECK(hipMemcpyAsync(dbuf, out.data(), n * sizeof(T), hipMemcpyHostToDevice, st));
  VO_HIP_CHECK(hipStreamSynchronize(st));
}
template void Comm::allreduce<int32_t>(int32_t*, size_t, bool, hipStream_t);
template void Comm::allreduce<double>(double*, size_t, bool, hipStream_t);

void comm_unique_id(char out[128]) {
  ncclUniqueId id;
  VO_NCCL_CHECK(ncclGetUniqueId(&id));
  static_assert(sizeof(id) == 128, "unexpected ncclUniqueId size");
  memcpy(out, &id, 128);
}

void comm_init_loopback(vo_ctx* ctx, int nranks, int rank, const char id[128]) {
  VO_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, VO_ERR_ARG, "vo_comm_init_loopback: bad rank");
  static std::mutex reg_mu;
  static std::map<std::string, std::weak_ptr<LoopGroup>> reg;
  std::shared_ptr<LoopGroup> g;
  {
    std::lock_guard<std::mutex> lk(reg_mu);
    const std::string key(id, 128);
    g = reg[key].lock();
    if (!g) {
      g = std::make_shared<LoopGroup>();
      g->nranks = nranks;
      g->slot.resize(nranks);
      reg[key] = g;
    }
  }
  VO_REQUIRE(g->nranks == nranks, VO_ERR_ARG, "vo_comm_init_loopback: group size mismatch");
  std::unique_ptr<Comm> c(new Comm);
  c->nranks = nranks;
  c->rank = rank;
  c->loop = g;
  ctx->comm = std::move(c);
}

void comm_init(vo_ctx* ctx, int nranks, int rank, const char id[128]) {
  VO_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, VO_ERR_ARG, "vo_comm_init: bad rank");
  std::unique_ptr<Comm> c(new Comm);
  c->nranks = nranks;
  c->rank = rank;
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  VO_NCCL_CHECK(ncclCommInitRank(&c->comm, nranks, uid, rank));
  ctx->comm = std::move(c);
}

}  // namespace vo
