// stats_merge_test.cpp — the merge of per-pass statistics and the "frame is still delivered" predicate
// (raingun_amd/csrc/rg_stats_merge.h) on the CPU: sums over one, two and three passes, no failure, one
// failing pass in each position, two failures at different pixels in both orders, two failures at one pixel
// (the earlier pass wins), indices past 2^31, and rg_delivers_frame over every status of include/raingun.h.
// Stand-alone; tests/test_stats_merge.py builds it with AddressSanitizer + UBSan and runs it.
// Prints "ok" and exits 0, or names the first failing check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raingun_amd/csrc/rg_stats_merge.h"

#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

struct pass {
    uint64_t primary, shadow, secondary;
    rg_status st;
    int32_t pixel;  // what rg_snap_status leaves: -1 without a failure
};

struct merged {
    rg_stats total;
    rg_status st;
};

// The fold every caller writes: a zeroed total with error_pixel -1 and RG_OK, then the passes in order.
static merged fold(const std::vector<pass> &passes) {
    merged m{};
    m.total.error_pixel = -1;
    m.total.kernel_ms = 7.5f;  // the caller's business: the merge leaves it alone
    m.st = RG_OK;
    for (const pass &p : passes) {
        rg_stats s{};
        s.rays.primary = p.primary;
        s.rays.shadow = p.shadow;
        s.rays.secondary = p.secondary;
        s.kernel_ms = 100.0f;
        s.error_pixel = p.pixel;
        rg_stats_add(m.total, m.st, s, p.st);
    }
    return m;
}

static void expect(const std::vector<pass> &passes, rg_status st, int32_t pixel, const char *what) {
    const merged m = fold(passes);
    uint64_t a = 0, b = 0, c = 0;
    for (const pass &p : passes) {
        a += p.primary;
        b += p.shadow;
        c += p.secondary;
    }
    CHECK(m.total.rays.primary == a && m.total.rays.shadow == b && m.total.rays.secondary == c, "%s: sums", what);
    CHECK(m.st == st, "%s: status %d, expected %d", what, (int)m.st, (int)st);
    CHECK(m.total.error_pixel == pixel, "%s: pixel %d, expected %d", what, (int)m.total.error_pixel, (int)pixel);
    CHECK(m.total.kernel_ms == 7.5f, "%s: kernel_ms touched", what);
}

int main() {
    const pass ok1{10, 20, 30, RG_OK, -1}, ok2{1ull << 40, 5, 0, RG_OK, -1}, ok3{7, 0, 9, RG_OK, -1};
    const pass nan5{3, 4, 5, RG_ERR_NAN_DISTANCE, 5}, aabb5{6, 7, 8, RG_ERR_AABB_NORMAL, 5};
    const pass aabb9{6, 7, 8, RG_ERR_AABB_NORMAL, 9}, tr2{1, 1, 1, RG_ERR_TRANSMISSION, 2};
    const pass nan0{2, 2, 2, RG_ERR_NAN_DISTANCE, 0};

    // sums over 1, 2 and 3 passes; no failure: RG_OK and pixel -1
    expect({}, RG_OK, -1, "no pass");
    expect({ok1}, RG_OK, -1, "one pass");
    expect({ok1, ok2}, RG_OK, -1, "two passes");
    expect({ok1, ok2, ok3}, RG_OK, -1, "three passes");
    // one failing pass in each position
    expect({nan5}, RG_ERR_NAN_DISTANCE, 5, "alone");
    expect({nan5, ok1, ok2}, RG_ERR_NAN_DISTANCE, 5, "first of three");
    expect({ok1, nan5, ok2}, RG_ERR_NAN_DISTANCE, 5, "second of three");
    expect({ok1, ok2, nan5}, RG_ERR_NAN_DISTANCE, 5, "third of three");
    expect({ok1, nan0}, RG_ERR_NAN_DISTANCE, 0, "pixel 0");
    // two failures at different pixels, in both orders: the lower pixel
    expect({nan5, aabb9}, RG_ERR_NAN_DISTANCE, 5, "lower first");
    expect({aabb9, nan5}, RG_ERR_NAN_DISTANCE, 5, "lower second");
    expect({aabb9, ok1, tr2}, RG_ERR_TRANSMISSION, 2, "lower third");
    expect({tr2, aabb9, nan5}, RG_ERR_TRANSMISSION, 2, "lowest first of three");
    expect({aabb9, nan5, tr2}, RG_ERR_TRANSMISSION, 2, "descending");
    // two failures at one pixel with different statuses: the earlier pass wins
    expect({nan5, aabb5}, RG_ERR_NAN_DISTANCE, 5, "tie, NaN first");
    expect({aabb5, nan5}, RG_ERR_AABB_NORMAL, 5, "tie, AABB first");
    expect({ok1, aabb5, nan5}, RG_ERR_AABB_NORMAL, 5, "tie behind a clean pass");
    // a sample frame's index may pass 2^31 (error_pixel is the u32 narrowed to i32): still the lower index
    const pass low{1, 0, 0, RG_ERR_NAN_DISTANCE, 0x7FFFFFF0}, high{1, 0, 0, RG_ERR_AABB_NORMAL, (int32_t)0x80000005u};
    expect({low, high}, RG_ERR_NAN_DISTANCE, 0x7FFFFFF0, "past 2^31, lower first");
    expect({high, low}, RG_ERR_NAN_DISTANCE, 0x7FFFFFF0, "past 2^31, lower second");
    expect({high}, RG_ERR_AABB_NORMAL, (int32_t)0x80000005u, "past 2^31 alone");

    // rg_delivers_frame: RG_OK and the reference's three panics, of every status of include/raingun.h
    const struct {
        rg_status st;
        bool delivers;
    } all[] = {{RG_OK, true},
               {RG_ERR_INVALID_ARGUMENT, false},
               {RG_ERR_PORTRAIT, false},
               {RG_ERR_AABB_NORMAL, true},
               {RG_ERR_NAN_DISTANCE, true},
               {RG_ERR_TRANSMISSION, true},
               {RG_ERR_TEXTURE, false},
               {RG_ERR_DEVICE, false},
               {RG_ERR_OUT_OF_MEMORY, false},
               {RG_ERR_CANCELLED, false},
               {RG_ERR_COLLECTIVE, false},
               {RG_ERR_PENDING, false}};
    for (const auto &e : all)
        CHECK(rg_delivers_frame(e.st) == e.delivers, "rg_delivers_frame(%d)", (int)e.st);
    for (int st = -16; st <= 1; ++st) {  // and nothing between them (the enumeration's value range)
        const bool want = st == RG_OK || st == RG_ERR_AABB_NORMAL || st == RG_ERR_NAN_DISTANCE || st == RG_ERR_TRANSMISSION;
        CHECK(rg_delivers_frame((rg_status)st) == want, "rg_delivers_frame(%d)", st);
    }
    std::printf("ok\n");
    return 0;
}
