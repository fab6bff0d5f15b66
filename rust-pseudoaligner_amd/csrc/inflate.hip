// pa_bgzf_inflate_device: BGZF members inflated on the GPU, one wave per member (blocks of one wave, grid-stride over the members).
// The decoder is csrc/inflate_core.hpp, shared with the host checker; here are the parts that need the wave: the barrier, the XOR reduction,
// staging the payload window into LDS with whole 16-byte loads where the member's own bytes allow it, and the launch.
#include <hip/hip_runtime.h>

#include "inflate_core.hpp"
#include "pa_common.hpp"

using namespace pa;
using namespace pa_inflate;

namespace {

constexpr uint32_t MAX_BLOCKS = 256 * 8;   // CUs x one-wave blocks per CU (two per SIMD): more members than this are taken grid-stride

struct WaveEnv {
    const uint8_t* comp;   // the member's payload
    uint32_t in_len;
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ uint32_t lanes() const { return 64; }
    // one wave per block: the barrier orders LDS and global accesses among the lanes (workgroup-scope release / acquire)
    __device__ void sync() const { __syncthreads(); }
    __device__ uint32_t xor_all(uint32_t v) const {
        for (int o = 32; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
        return v;
    }
    __device__ uint8_t payload(uint32_t i) const { return i < in_len ? comp[i] : (uint8_t)0; }
    __device__ void stage(uint8_t* win, int32_t origin) const {
        const bool aligned = (((uintptr_t)(comp + origin)) & 15u) == 0;   // (pointer arithmetic only: nothing is loaded outside [0, in_len))
        for (uint32_t g = threadIdx.x; g < IN_WIN / 16; g += 64) {
            const int64_t at = (int64_t)origin + 16 * (int64_t)g;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (aligned && at >= 0 && at + 16 <= (int64_t)in_len) {
                v = *reinterpret_cast<const uint4*>(comp + at);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int b = 0; b < 16; b++) {
                    const int64_t i = at + b;
                    if (i >= 0 && i < (int64_t)in_len) w[b >> 2] |= (uint32_t)comp[i] << (8 * (b & 3));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(win + 16 * g) = v;
        }
    }
};

__global__ void __launch_bounds__(64) pa_bgzf_inflate_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes, const pa_bgzf_member* __restrict__ members, uint64_t n_members,
                                                             uint8_t* text, uint64_t text_cap, uint32_t* __restrict__ status) {
    __shared__ Work w;
    const uint64_t base = members[0].out_off;
    for (uint64_t i = blockIdx.x; i < n_members; i += gridDim.x) {
        const pa_bgzf_member m = members[i];
        uint32_t st = PA_INFLATE_BAD_MEMBER, crc = 0;
        // the row is checked before anything of the member is touched: payload inside comp, text inside text_cap
        if (m.out_len <= PA_BGZF_MAX_ISIZE && m.in_off <= comp_bytes && m.in_len <= comp_bytes - m.in_off && m.out_off >= base && m.out_off - base <= text_cap &&
            m.out_len <= text_cap - (m.out_off - base)) {
            WaveEnv env{comp + m.in_off, m.in_len};
            st = inflate_member(env, w, m.in_len, text + (m.out_off - base), m.out_len, m.crc32, -(int32_t)((uintptr_t)(comp + m.in_off) & 15u), &crc);
        }
        __syncthreads();   // the next member reuses the LDS
        if (threadIdx.x == 0) status[i] = st;
    }
}

}  // namespace

extern "C" const char* pa_inflate_status_name(uint32_t status) {
    static const char* const NAMES[] = {"ok", "inconsistent member table row", "reserved block type", "stored block length check", "too many length or distance symbols",
                                        "invalid code lengths", "invalid code length repeat", "missing end-of-block code", "invalid symbol", "distance too far back",
                                        "input exhausted", "bytes behind the end of the stream", "more text than ISIZE", "less text than ISIZE", "crc mismatch"};
    return status < sizeof(NAMES) / sizeof(NAMES[0]) ? NAMES[status] : "unknown";
}

extern "C" int pa_bgzf_inflate_device(int device, const uint8_t* d_comp, uint64_t comp_bytes, const pa_bgzf_member* d_members, uint64_t n_members, uint8_t* d_text,
                                      uint64_t text_cap, uint32_t* d_status, void* stream) {
    if (n_members == 0) return PA_OK;
    if (!d_comp || !d_members || !d_status || (text_cap && !d_text)) return fail(PA_ERR_INVALID_ARG, "pa_bgzf_inflate_device: null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        return fail(PA_ERR_NO_DEVICE, "no HIP device: members are inflated on the GPU, there is no CPU fallback");
    }
    if (hipSetDevice(device) != hipSuccess) return fail(PA_ERR_HIP, "hipSetDevice(%d) failed", device);
    return bgzf_inflate_launch(d_comp, comp_bytes, d_members, n_members, d_text, text_cap, d_status, stream);
}

int pa::bgzf_inflate_launch(const uint8_t* d_comp, uint64_t comp_bytes, const pa_bgzf_member* d_members, uint64_t n_members, uint8_t* d_text, uint64_t text_cap,
                            uint32_t* d_status, void* stream) {
    if (n_members == 0) return PA_OK;
    const uint32_t blocks = (uint32_t)(n_members < MAX_BLOCKS ? n_members : MAX_BLOCKS);
    hipLaunchKernelGGL(pa_bgzf_inflate_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), d_comp, comp_bytes, d_members, n_members, d_text, text_cap, d_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PA_ERR_HIP, "pa_bgzf_inflate_device: launch failed: %s", hipGetErrorString(e));
    return PA_OK;
}
