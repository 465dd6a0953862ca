// rg_rccl.hip — the run-time RCCL loader (rg_rccl.h) and the communicators of N processes
// (rg_comm_*, include/raingun_frames.h).
#include "rg_rccl.h"

#include <dlfcn.h>
#include <link.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/raingun.h"
#include "rg_internal.h"

namespace {

Rccl g_rccl;
std::mutex g_rccl_mu;

int find_loaded(struct dl_phdr_info *info, size_t, void *data) {
    if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) {
        *static_cast<std::string *>(data) = info->dlpi_name;
        return 1;
    }
    return 0;
}

}  // namespace

const Rccl *rccl_loaded() { return g_rccl.handle ? &g_rccl : nullptr; }

const Rccl *rccl() {
    std::lock_guard<std::mutex> g(g_rccl_mu);
    if (g_rccl.tried) return rccl_loaded();
    g_rccl.tried = true;
    std::string loaded;
    dl_iterate_phdr(find_loaded, &loaded);
    std::vector<std::string> cands;
    if (!loaded.empty()) cands.push_back(loaded);  // the instance already in the process (e.g. PyTorch's)
    if (const char *e = std::getenv("RG_RCCL_LIBRARY")) cands.push_back(e);
    cands.push_back("librccl.so.1");
    cands.push_back("/opt/rocm/lib/librccl.so.1");
    for (const std::string &c : cands) {
        void *h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) continue;
        g_rccl.init_all = reinterpret_cast<pfn_comm_init_all>(dlsym(h, "ncclCommInitAll"));
        g_rccl.destroy = reinterpret_cast<pfn_comm_destroy>(dlsym(h, "ncclCommDestroy"));
        g_rccl.gather = reinterpret_cast<pfn_gather>(dlsym(h, "ncclGather"));
        g_rccl.group_start = reinterpret_cast<pfn_group>(dlsym(h, "ncclGroupStart"));
        g_rccl.group_end = reinterpret_cast<pfn_group>(dlsym(h, "ncclGroupEnd"));
        g_rccl.get_unique_id = reinterpret_cast<pfn_get_unique_id>(dlsym(h, "ncclGetUniqueId"));
        g_rccl.init_rank = reinterpret_cast<pfn_comm_init_rank>(dlsym(h, "ncclCommInitRank"));
        g_rccl.count = reinterpret_cast<pfn_comm_query>(dlsym(h, "ncclCommCount"));
        g_rccl.cu_device = reinterpret_cast<pfn_comm_query>(dlsym(h, "ncclCommCuDevice"));
        g_rccl.user_rank = reinterpret_cast<pfn_comm_query>(dlsym(h, "ncclCommUserRank"));
        if (g_rccl.init_all && g_rccl.destroy && g_rccl.gather && g_rccl.group_start && g_rccl.group_end &&
            g_rccl.get_unique_id && g_rccl.init_rank && g_rccl.count && g_rccl.cu_device && g_rccl.user_rank) {
            g_rccl.handle = h;
            return &g_rccl;
        }
        dlclose(h);
    }
    return nullptr;
}

// ---------------------------------------------------------------- communicators of N processes
// (include/raingun_frames.h): the library's own RCCL communicator for the
// one-process-per-GPU frame loop -- rank 0 makes the unique id, the caller
// hands it to every rank (any channel: torch.distributed's store, MPI, a file),
// and every rank joins with ncclCommInitRank on its device.  No torch internals.
extern "C" {

int32_t rg_comm_id_bytes(void) { return RG_COMM_ID_BYTES; }

rg_status rg_comm_unique_id(uint8_t *id) {
    if (!id) return RG_ERR_INVALID_ARGUMENT;
    const Rccl *r = rccl();
    if (!r) return RG_ERR_COLLECTIVE;
    NcclUniqueId u;
    if (r->get_unique_id(&u) != 0) return RG_ERR_COLLECTIVE;
    std::memcpy(id, u.internal, sizeof u.internal);
    return RG_OK;
}

rg_status rg_comm_init_rank(const uint8_t *id, int32_t world, int32_t rank, int32_t device, void **comm) {
    if (!comm) return RG_ERR_INVALID_ARGUMENT;
    *comm = nullptr;
    if (!id || world < 1 || rank < 0 || rank >= world || device < 0) return RG_ERR_INVALID_ARGUMENT;
    const Rccl *r = rccl();
    if (!r) return RG_ERR_COLLECTIVE;
    int ndev = 0;
    if (!ok(hipGetDeviceCount(&ndev)) || device >= ndev) return RG_ERR_INVALID_ARGUMENT;
    if (!ok(hipSetDevice(device))) return RG_ERR_DEVICE;  // ncclCommInitRank binds the current device
    NcclUniqueId u;
    std::memcpy(u.internal, id, sizeof u.internal);
    void *c = nullptr;
    if (r->init_rank(&c, world, u, rank) != 0 || !c) return RG_ERR_COLLECTIVE;
    *comm = c;
    return RG_OK;
}

rg_status rg_comm_info(void *comm, int32_t *nranks, int32_t *rank, int32_t *device) {
    const Rccl *r = rccl_loaded();
    if (!comm || !r) return RG_ERR_INVALID_ARGUMENT;
    const std::pair<pfn_comm_query, int32_t *> q[3] = {{r->count, nranks}, {r->user_rank, rank}, {r->cu_device, device}};
    for (const auto &e : q) {
        int v = 0;
        if (!e.second) continue;
        if (e.first(comm, &v) != 0) return RG_ERR_COLLECTIVE;
        *e.second = v;
    }
    return RG_OK;
}

rg_status rg_comm_destroy(void *comm) {
    const Rccl *r = rccl_loaded();
    if (!comm || !r) return RG_ERR_INVALID_ARGUMENT;
    return r->destroy(comm) == 0 ? RG_OK : RG_ERR_COLLECTIVE;
}

rg_gather_fn rg_comm_gather_fn(void) {
    const Rccl *r = rccl();
    return r ? reinterpret_cast<rg_gather_fn>(r->gather) : nullptr;
}

}  // extern "C"
