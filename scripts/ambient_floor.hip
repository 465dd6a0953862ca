// ambient_floor.hip — the memory floors scripts/ambient_bench.py compares the ambient term's two image kernels
// with: streaming kernels that move the same bytes per pixel and do nothing else.  Built by the script into
// scripts/bin/libambient_floor.so (hipcc --offload-arch=gfx950 -O3 -shared -fPIC); not part of the library.
//   ambient_floor_filter:  reads ao (4 B), body (4 B) and normal (12 B), writes 4 B per pixel
//   ambient_floor_compose: reads rgb (12 B), albedo (12 B), body (4 B) and aof (4 B), writes 4 B per pixel
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__global__ __launch_bounds__(256) void floor_filter(const float *ao, const int32_t *body, const float *normal, float *out,
                                                    unsigned long long npx) {
    const unsigned long long o = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (o >= npx) return;
    out[o] = ao[o] + (float)body[o] + normal[3 * o] + normal[3 * o + 1] + normal[3 * o + 2];
}

__global__ __launch_bounds__(256) void floor_compose(const float *rgb, const float *albedo, const int32_t *body,
                                                     const float *aof, uint32_t *rgba, unsigned long long npx) {
    const unsigned long long o = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (o >= npx) return;
    float s = aof[o] + (float)body[o];
    for (int c = 0; c < 3; ++c) s += rgb[3 * o + c] + albedo[3 * o + c];
    rgba[o] = __float_as_uint(s);
}

}  // namespace

extern "C" int ambient_floor_filter(const float *ao, const int32_t *body, const float *normal, float *out,
                                    unsigned long long npx, void *stream) {
    if (!ao || !body || !normal || !out || npx == 0 || npx >= (1ull << 32)) return 1;
    hipLaunchKernelGGL(floor_filter, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), ao,
                       body, normal, out, npx);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int ambient_floor_compose(const float *rgb, const float *albedo, const int32_t *body, const float *aof,
                                     uint32_t *rgba, unsigned long long npx, void *stream) {
    if (!rgb || !albedo || !body || !aof || !rgba || npx == 0 || npx >= (1ull << 32)) return 1;
    hipLaunchKernelGGL(floor_compose, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rgb,
                       albedo, body, aof, rgba, npx);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
