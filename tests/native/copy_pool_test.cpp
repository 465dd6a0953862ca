// copy_pool_test.cpp — stand-alone CPU check of rg_copy_pool (raingun_amd/csrc/rg_copy_pool.cpp),
// meant to be built with -fsanitize=thread and with -fsanitize=address,undefined
// (tests/test_copy_pool.py).  For 0, 1 and 3 helpers, three rounds each: copies between begin()
// and end() (helpers spinning) of sizes around the inline-memcpy threshold (256 KiB), the 4-KiB
// piece rounding and a last piece that is empty or short; then, after end(), one 1-MiB copy
// that has to wake the helpers from their condition variable.  Every copy is compared byte for
// byte, and 32 guard bytes on either side of the destination must stay untouched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raingun_amd/csrc/rg_copy_pool.h"

namespace {

const size_t GUARD = 32;
int failures = 0;

void check_copy(rg_copy_pool &pool, size_t bytes, uint32_t salt) {
    std::vector<unsigned char> src(bytes + 1), dst(bytes + 2 * GUARD);  // + 1: a valid pointer for 0 bytes
    uint32_t x = salt * 2654435761u + 1u;
    for (size_t i = 0; i < bytes; ++i) {
        x = x * 1664525u + 1013904223u;
        src[i] = (unsigned char)(x >> 24);
    }
    std::memset(dst.data(), 0xA5, dst.size());
    pool.copy(dst.data() + GUARD, src.data(), bytes);
    bool good = bytes == 0 || std::memcmp(dst.data() + GUARD, src.data(), bytes) == 0;
    for (size_t i = 0; i < GUARD; ++i) good = good && dst[i] == 0xA5 && dst[GUARD + bytes + i] == 0xA5;
    if (!good) {
        std::fprintf(stderr, "copy of %zu bytes (salt %u): wrong bytes or guard overwritten\n", bytes, salt);
        ++failures;
    }
}

}  // namespace

int main() {
    const size_t K = 1024, M = 1024 * K;
    const size_t sizes[] = {0, 1, 4095, 4096, 256 * K - 1, 256 * K, 256 * K + 1, M + 4097, 3 * M};
    const int helpers[] = {0, 1, 3};
    uint32_t salt = 0;
    for (int h : helpers) {
        rg_copy_pool pool(h);
        for (int round = 0; round < 3; ++round) {
            {
                rg_copy_pool::Active active(pool);
                for (size_t n : sizes) check_copy(pool, n, ++salt);
            }
            check_copy(pool, M, ++salt);  // helpers asleep (or on their way): woken by the new generation
        }
    }
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
