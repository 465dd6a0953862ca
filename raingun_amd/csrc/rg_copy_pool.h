// rg_copy_pool.h — parallel host memcpy of the host-visible frame paths
// (rg_capi.hip, rg_multi.hip).  Plain C++: no HIP header, so the pool also
// builds as a stand-alone CPU program (tests/native/copy_pool_test.cpp).
#pragma once
#include <cstddef>

#ifndef RG_COPY_HELPERS
#define RG_COPY_HELPERS 3       // helper threads of the pageable host copy (plus the calling thread)
#endif

// Parallel host memcpy for frames delivered into PAGEABLE caller memory: one
// thread moves a band out of pinned staging at ~10-17 GB/s, a third of what
// PCIe delivers (~56 GB/s), so the band is split over the calling thread and
// RG_COPY_HELPERS helpers.  Helpers spin while a render call is in progress
// (fork/join per band in ~1 us) and sleep between calls.
class rg_copy_pool {
  public:
    explicit rg_copy_pool(int helpers);
    ~rg_copy_pool();
    rg_copy_pool(const rg_copy_pool &) = delete;
    rg_copy_pool &operator=(const rg_copy_pool &) = delete;
    void begin();  // a render call starts: helpers spin
    void end();    // ... ends: helpers sleep
    void copy(void *dst, const void *src, size_t bytes);  // blocking, split over all threads

    // begin() now, end() on every way out of the render call's scope
    struct Active {
        rg_copy_pool &p;
        explicit Active(rg_copy_pool &q) : p(q) { p.begin(); }
        ~Active() { p.end(); }
        Active(const Active &) = delete;
        Active &operator=(const Active &) = delete;
    };

  private:
    void run(int id);
    struct Impl;
    Impl *p_;
};
