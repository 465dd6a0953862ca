// rg_rccl.h — RCCL, loaded at run time (rg_rccl.hip): libraingun_hip.so links no collective
// library and shares the one already in a process (PyTorch's) if there is one.  The loader
// serves rg_render_multi's gather mode (rg_multi.hip) and the rg_comm_* functions of
// include/raingun_frames.h, which rg_rccl.hip defines.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/raingun_frames.h"

#pragma GCC visibility push(hidden)

typedef int (*pfn_comm_init_all)(void **comms, int ndev, const int *devlist);
typedef int (*pfn_comm_destroy)(void *comm);
typedef int (*pfn_gather)(const void *send, void *recv, size_t count, int dtype, int root, void *comm, hipStream_t s);
typedef int (*pfn_group)(void);
struct NcclUniqueId {  // ncclUniqueId (rccl.h): 128 opaque bytes, passed by value to ncclCommInitRank
    char internal[RG_COMM_ID_BYTES];
};
typedef int (*pfn_get_unique_id)(NcclUniqueId *id);
typedef int (*pfn_comm_init_rank)(void **comm, int nranks, NcclUniqueId id, int rank);
typedef int (*pfn_comm_query)(void *comm, int *out);  // ncclCommCount / ncclCommCuDevice / ncclCommUserRank

struct Rccl {
    bool tried = false;
    void *handle = nullptr;
    pfn_comm_init_all init_all = nullptr;
    pfn_comm_destroy destroy = nullptr;
    pfn_gather gather = nullptr;
    pfn_group group_start = nullptr, group_end = nullptr;
    pfn_get_unique_id get_unique_id = nullptr;
    pfn_comm_init_rank init_rank = nullptr;
    pfn_comm_query count = nullptr, cu_device = nullptr, user_rank = nullptr;
};

const Rccl *rccl();         // loaded on first use; nullptr: no usable library
const Rccl *rccl_loaded();  // the loader if it is already loaded, else nullptr: never loads

constexpr int kNcclUint8 = 1;       // ncclDataType_t (rccl.h)
constexpr int kNcclInProgress = 7;  // a non-blocking communicator's "enqueued"

#pragma GCC visibility pop
