// ambient_test.cpp -- raingun_amd/csrc/rg_ambient.h as a stand-alone program (tests/test_ambient_cpu.py builds it
// twice: plain, and with AddressSanitizer + UBSan as its own executable).  The header's filter against a
// restatement that first lists a pixel's accepted taps and then adds them up, over frames smaller than the window
// (1x1, 3x2, 17x3 at every radius), with NaN normals, zero normals and pixels without a body; the validity
// predicates; the share of every surface kind; the compose's clamp and bytes.  Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raingun_amd/csrc/rg_ambient.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Frame {
    uint32_t w, h;
    std::vector<float> ao, normal;
    std::vector<int32_t> body;
};

Frame make_frame(uint32_t w, uint32_t h, uint32_t seed) {
    Frame f{w, h, std::vector<float>((size_t)w * h), std::vector<float>((size_t)w * h * 3), std::vector<int32_t>((size_t)w * h)};
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t p = 0; p < (size_t)w * h; ++p) {
        f.ao[p] = (float)(lcg(seed) >> 8) / 16777216.0f;
        const uint32_t r = lcg(seed) >> 16;
        f.body[p] = r % 11 == 0 ? -1 : (int32_t)(r % 3);
        const float scale = 0.25f + (float)(lcg(seed) >> 24) / 64.0f;  // not unit
        f.normal[3 * p] = scale * ((float)(lcg(seed) >> 24) / 1024.0f);
        f.normal[3 * p + 1] = scale * (1.0f + (float)(lcg(seed) >> 24) / 1024.0f);
        f.normal[3 * p + 2] = scale * ((r & 1) ? 0.3f : -0.3f);
        if (r % 13 == 0) f.normal[3 * p + (r % 3)] = nan;
        if (r % 17 == 0) f.normal[3 * p] = f.normal[3 * p + 1] = f.normal[3 * p + 2] = 0.0f;
    }
    return f;
}

// the contract once more: list the accepted taps in order, then add them up
float restated(const Frame &f, uint32_t radius, float nmin, uint32_t x, uint32_t y) {
    const size_t p = (size_t)y * f.w + x;
    if (f.body[p] < 0) return f.ao[p];
    struct Tap {
        int w;
        float ao;
    };
    std::vector<Tap> taps;
    const int r = (int)radius;
    const float *np = &f.normal[3 * p];
    const float nn_p = (np[0] * np[0] + np[1] * np[1]) + np[2] * np[2], t = nmin * nmin;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)f.w || qy >= (int)f.h) continue;
            const size_t q = (size_t)qy * f.w + (size_t)qx;
            const float *nq = &f.normal[3 * q];
            const float d = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
            const float nn_q = (nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2];
            const bool centre = dx == 0 && dy == 0;
            if (centre || (f.body[q] == f.body[p] && d > 0.0f && d * d >= t * (nn_p * nn_q)))
                taps.push_back({(r + 1 - std::abs(dx)) * (r + 1 - std::abs(dy)), f.ao[q]});
        }
    float sum = 0.0f;
    int wsum = 0;
    for (const Tap &tap : taps) {
        sum = sum + (float)tap.w * tap.ao;
        wsum += tap.w;
    }
    CHECK(wsum >= (r + 1) * (r + 1) && wsum <= 6561);
    return sum / (float)wsum;
}

void test_filter() {
    const uint32_t sizes[][2] = {{1, 1}, {3, 2}, {17, 3}, {2, 19}, {23, 21}};
    const float nmins[] = {0.0f, 0.9f, 1.0f};
    for (const auto &s : sizes) {
        const Frame f = make_frame(s[0], s[1], 12345u + s[0] * 31u + s[1]);
        for (uint32_t r = 1; r <= RG_AO_FILTER_MAX_RADIUS; ++r)
            for (float nmin : nmins)
                for (uint32_t y = 0; y < f.h; ++y)
                    for (uint32_t x = 0; x < f.w; ++x) {
                        const float got = rg_ao_filter_pixel(f.ao.data(), f.body.data(), f.normal.data(), f.w, f.h, r, nmin, x, y);
                        CHECK(bits(got) == bits(restated(f, r, nmin, x, y)));
                        if (f.body[(size_t)y * f.w + x] < 0) CHECK(bits(got) == bits(f.ao[(size_t)y * f.w + x]));
                    }
    }
    // a centre whose own normal is NaN accepts nothing but itself: the result is w * ao / w
    Frame f = make_frame(5, 5, 7u);
    const size_t c = 2 * 5 + 2;
    f.body.assign(25, 0);
    f.normal[3 * c] = std::numeric_limits<float>::quiet_NaN();
    const float got = rg_ao_filter_pixel(f.ao.data(), f.body.data(), f.normal.data(), 5, 5, 2, 0.0f, 2, 2);
    CHECK(bits(got) == bits((9.0f * f.ao[c]) / 9.0f));
    // weights
    CHECK(rg_ao_filter_weight(8, 0, 0) == 81 && rg_ao_filter_weight(8, -8, 8) == 1 && rg_ao_filter_weight(2, -1, 2) == 2);
    int total = 0;
    for (int dy = -8; dy <= 8; ++dy)
        for (int dx = -8; dx <= 8; ++dx) total += rg_ao_filter_weight(8, dx, dy);
    CHECK(total == 6561);
}

void test_valid() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(rg_ao_filter_valid(1, 0.0f) && rg_ao_filter_valid(8, 1.0f) && rg_ao_filter_valid(2, 0.9f));
    CHECK(!rg_ao_filter_valid(0, 0.9f) && !rg_ao_filter_valid(9, 0.9f) && !rg_ao_filter_valid(2, nan));
    CHECK(!rg_ao_filter_valid(2, -0.01f) && !rg_ao_filter_valid(2, 1.01f) && !rg_ao_filter_valid(2, inf));
    const float good[3] = {0.0f, 0.5f, 7.0f}, neg[3] = {0.1f, -0.1f, 0.1f}, bad[3] = {0.1f, nan, 0.1f}, big[3] = {inf, 0.0f, 0.0f};
    CHECK(rg_ambient_valid(good, 1, 0, 0.9f) && rg_ambient_valid(good, 8, 8, 1.0f));
    CHECK(!rg_ambient_valid(neg, 1, 2, 0.9f) && !rg_ambient_valid(bad, 1, 2, 0.9f) && !rg_ambient_valid(big, 1, 2, 0.9f));
    CHECK(!rg_ambient_valid(good, 0, 2, 0.9f) && !rg_ambient_valid(good, 9, 2, 0.9f) && !rg_ambient_valid(good, 1, 9, 0.9f));
    CHECK(!rg_ambient_valid(good, 1, 2, nan) && !rg_ambient_valid(good, 1, 2, 1.5f));
}

void test_share_and_compose() {
    CHECK(bits(rg_ambient_share(0, 0.18f, 0.7f)) == bits(0.18f));
    CHECK(bits(rg_ambient_share(1, 0.18f, 0.7f)) == bits((1.0f - 0.7f) * 0.18f));
    CHECK(bits(rg_ambient_share(2, 0.18f, 0.7f)) == bits(0.0f));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(rg_ambient_clamp(-0.5f) == 0.0f && rg_ambient_clamp(1.5f) == 1.0f && rg_ambient_clamp(nan) == 0.0f);
    CHECK(bits(rg_ambient_clamp(0.25f)) == bits(0.25f));
    CHECK(bits(rg_ambient_channel(0.25f, 0.0f, 0.8f, 0.5f, 0.75f, true)) == bits(0.25f));   // colour 0: the beauty frame
    CHECK(bits(rg_ambient_channel(0.25f, 0.3f, 0.8f, 0.5f, 0.75f, false)) == bits(0.25f));  // a miss
    CHECK(bits(rg_ambient_channel(0.25f, 0.3f, 0.8f, 0.5f, 0.75f, true)) == bits(0.25f + (0.3f * 0.8f) * (0.5f * 0.75f)));
    CHECK(rg_ambient_channel(0.9f, 1.0f, 1.0f, 1.0f, 1.0f, true) == 1.0f);
    CHECK(rg_ambient_u8(0.0f) == 0 && rg_ambient_u8(1.0f) == 255 && rg_ambient_u8(0.5f) == 127 && rg_ambient_u8(nan) == 0);
}

}  // namespace

int main() {
    test_filter();
    test_valid();
    test_share_and_compose();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
