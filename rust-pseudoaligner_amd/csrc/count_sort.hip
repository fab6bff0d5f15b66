// The equivalence-class count table (the unit the GPUs of a node reduce over RCCL) from the KEY STREAMS of a
// mapping launch. The map kernel (map_pool.hip) appends one key per finished read — the slot of the table the read counts
// in — to its wave's stream; the streams are fully coalesced writes (0.4 GB per 100 M reads). Here:
//
//   one bin  (table of <= 32768 slots, e.g. gencode_small)     pa_keys_count_kernel straight over the streams
//   several  pa_keys_part_kernel     keys partitioned by bin (bin = key >> 15: 32768 consecutive slots = 128 KiB of LDS counters)
//                                    inside tiles, one read of the stream: a workgroup counts its tile's keys per bin in LDS and
//                                    writes the tile's runs — as 16-bit keys, the run names the bin — to the tile's own slot of
//                                    `sorted`, whole lines; the map kernel's chunks while pa_resolve_kernel runs, the deferred
//                                    reads' keys after it
//            pa_keys_count_kernel    one LDS table per workgroup and bin: LDS atomics over its share of the bin's runs,
//                                    then the non-zero counters are added to the caller's u64 table
//
// Round 2 counted inside the map kernel with one device-scope atomic per read into per-XCD replicas of the table; the table
// (1.9 MB per replica at config 3) does not survive in an L2 that 3 GB of dictionary lines, node blobs and read tiles stream
// through per launch, and a device-scope atomic that misses is forwarded to the memory side: 100 M random 32-byte requests
// per 100 M reads, 8-9 % of the kernel. The same counts by sorting move 0.4 GB of coalesced reads and 2 x 0.2 GB of partitioned keys.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {
namespace {

constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
#ifndef PA_MAX_BINS
#define PA_MAX_BINS 256   // (-DPA_MAX_BINS=2: the test build in which a table of 100 k classes already is "beyond MAX_BINS", _build.build_maxbins_variant)
#endif
constexpr uint32_t MAX_BINS = PA_MAX_BINS;               // tables of up to 8.4 M slots; beyond, keys are counted with plain atomics
constexpr uint64_t PA_COUNT_DIRECT_MAX_READS = 1u << 16; // ... and so are the keys of batches this small
constexpr uint32_t BIN_SLOTS = 1u << PA_KEY_BIN_SHIFT;
constexpr uint32_t CS_BLOCK = 1024;

// The keys of a launch: what the waves of the map kernel appended (whole chunks of PA_KEY_CHUNK, *keys_top entries) and, right
// behind them in the same buffer, one key per deferred read from pa_resolve_kernel (resolve.hip: as many as the stream of deferred
// reads holds, a multiple of PA_DEFER_CHUNK; *extra_top, may be null). Both are multiples of four.
struct KeyTops {
    const unsigned long long* top;
    uint64_t cap;
    const unsigned long long* extra_top;
    uint64_t extra_cap;
};
__device__ __forceinline__ uint64_t stream_len(const KeyTops k, uint64_t unused = 0) {
    (void)unused;
    unsigned long long t = *k.top, x = k.extra_top ? *k.extra_top : 0ull;
    if (t > k.cap) t = k.cap;
    if (x > k.extra_cap) x = k.extra_cap;
    return t + x;
}

// Counting sort of the keys by bin in ONE pass over the stream, without a global atomic and without waiting on another workgroup:
// the stream is cut into tiles of PT_TILE keys, and tile t's keys, partitioned by bin inside LDS, go to tile t's own slot of
// `sorted` (sorted[t * PT_TILE ...], as 16-bit keys: the bin's run names the bin) — tile-major, not bin-major: a bin-major layout
// needs every bin's global base, that is the histogram of the WHOLE stream, before the first key can be written (the pass that
// reads the stream a second time). Where a tile's run of bin b lies is run_off[b * tcap + t] .. run_off[(b + 1) * tcap + t]
// (row nbins: the tile's key count). pa_keys_count_kernel then reads, per bin, the runs of that bin in every tile.
//   pass 0  the map kernel's chunks [0, *keys_top): needs only the map kernel (runs while pa_resolve_kernel appends its keys)
//   pass 1  the deferred reads' keys [*keys_top, + *extra_top): tiles numbered on behind those of pass 0
constexpr uint32_t PT_BLOCK = 512, PT_PER = 16, PT_TILE = PT_BLOCK * PT_PER;

__device__ __forceinline__ uint64_t main_len(const KeyTops k) { const unsigned long long t = *k.top; return t < k.cap ? t : k.cap; }
__device__ __forceinline__ uint64_t extra_len(const KeyTops k) {
    const unsigned long long x = k.extra_top ? *k.extra_top : 0ull;
    return x < k.extra_cap ? x : k.extra_cap;
}
__device__ __forceinline__ uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + PT_TILE - 1) / PT_TILE); }

__global__ __launch_bounds__(PT_BLOCK) void pa_keys_part_kernel(const uint32_t* __restrict__ keys, const KeyTops keys_top, uint32_t pass, uint32_t nbins,
                                                                uint32_t tcap, uint16_t* __restrict__ sorted, uint32_t* __restrict__ run_off) {
    __shared__ uint32_t cnt[MAX_BINS], lbase[MAX_BINS + 1];
    __shared__ __attribute__((aligned(16))) uint16_t stage[PT_TILE];
    const uint64_t m = main_len(keys_top);
    const uint64_t seg0 = pass ? m : 0, len = pass ? extra_len(keys_top) : m;   // (both multiples of four: 16-byte loads)
    const uint32_t tile0 = pass ? tiles_of(m) : 0u, ntiles = tiles_of(len);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (uint32_t b = threadIdx.x; b < nbins; b += PT_BLOCK) cnt[b] = 0;
        __syncthreads();
        const uint64_t t0 = (uint64_t)t * PT_TILE;
        uint32_t k[PT_PER], pos[PT_PER];
        const uint4* src = reinterpret_cast<const uint4*>(keys + seg0 + t0) + threadIdx.x;
#pragma unroll
        for (uint32_t j = 0; j < PT_PER / 4; ++j) {   // coalesced 16-byte loads, all in flight together
            const uint64_t i = t0 + 4ull * (j * PT_BLOCK + threadIdx.x);
            const uint4 v = i < len ? src[j * PT_BLOCK] : uint4{NO_KEY, NO_KEY, NO_KEY, NO_KEY};
            k[4 * j] = v.x; k[4 * j + 1] = v.y; k[4 * j + 2] = v.z; k[4 * j + 3] = v.w;
        }
#pragma unroll
        for (uint32_t j = 0; j < PT_PER; ++j) pos[j] = k[j] != NO_KEY ? atomicAdd(&cnt[k[j] >> PA_KEY_BIN_SHIFT], 1u) : 0u;   // rank inside the tile's run of that bin
        __syncthreads();
        for (uint32_t b = threadIdx.x; b <= nbins; b += PT_BLOCK) {
            uint32_t s = 0;
            for (uint32_t j = 0; j < b; ++j) s += cnt[j];
            lbase[b] = s;
            run_off[(uint64_t)b * tcap + tile0 + t] = s;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < PT_PER; ++j)
            if (k[j] != NO_KEY) stage[lbase[k[j] >> PA_KEY_BIN_SHIFT] + pos[j]] = (uint16_t)(k[j] & (BIN_SLOTS - 1));
        __syncthreads();
        // the tile's slot, whole 16-byte pieces from its start (what lies behind the last run is never read)
        uint4* dst = reinterpret_cast<uint4*>(sorted + (uint64_t)(tile0 + t) * PT_TILE);
        const uint32_t n8 = (lbase[nbins] + 7) / 8;
        for (uint32_t i = threadIdx.x; i < n8; i += PT_BLOCK) dst[i] = reinterpret_cast<const uint4*>(stage)[i];
        __syncthreads();
    }
}

// counts[(bin << 15) + i] += occurrences of key i in the bin's runs of `sorted` (16-bit keys). Workgroup (bin, part) takes part `part`
// of `parts` of the tiles; every 16-lane group of its waves takes one tile at a time and reads the tile's run of the bin in
// 16-byte pieces (eight keys; the few keys before the first and after the last aligned octet one by one).
constexpr uint32_t CG_LANES = 16, CG_DEPTH = 8;   // lanes per group; octets in flight per lane (one pass over a run of <= 1024 keys)
__global__ __launch_bounds__(CS_BLOCK) void pa_keys_count_kernel(const uint16_t* __restrict__ src, const uint32_t* __restrict__ run_off, uint32_t tcap,
                                                                 const KeyTops keys_top, uint32_t parts, unsigned long long* __restrict__ counts,
                                                                 uint64_t counts_len) {
    extern __shared__ uint32_t tab[];   // BIN_SLOTS counters
    const uint32_t bin = blockIdx.x / parts, part = blockIdx.x % parts;
    const uint64_t slot0 = (uint64_t)bin << PA_KEY_BIN_SHIFT;
    const uint32_t nslots = (uint32_t)(counts_len - slot0 < BIN_SLOTS ? counts_len - slot0 : BIN_SLOTS);
    for (uint32_t i = threadIdx.x; i < nslots; i += CS_BLOCK) tab[i] = 0;
    __syncthreads();
    const uint32_t ntiles = tiles_of(main_len(keys_top)) + tiles_of(extra_len(keys_top));
    const uint32_t ta = (uint32_t)((uint64_t)ntiles * part / parts), tb = (uint32_t)((uint64_t)ntiles * (part + 1) / parts);
    const uint32_t gl = threadIdx.x % CG_LANES, group = threadIdx.x / CG_LANES;
    const uint4* q = reinterpret_cast<const uint4*>(src);
    for (uint32_t t = ta + group; t < tb; t += CS_BLOCK / CG_LANES) {
        const uint64_t base = (uint64_t)t * PT_TILE;
        const uint64_t a = base + run_off[(uint64_t)bin * tcap + t], b = base + run_off[(uint64_t)(bin + 1) * tcap + t];
        const uint64_t a8 = (a + 7) & ~7ull, b8 = b & ~7ull;
        if (a8 >= b8) {
            for (uint64_t i = a + gl; i < b; i += CG_LANES) atomicAdd(&tab[src[i]], 1u);
            continue;
        }
        const uint32_t head = a + gl < a8 ? src[a + gl] : 0xFFFFu, tail = b8 + gl < b ? src[b8 + gl] : 0xFFFFu;
        for (uint64_t o0 = a8 / 8; o0 < b8 / 8; o0 += (uint64_t)CG_DEPTH * CG_LANES) {
            uint4 v[CG_DEPTH];
            bool in[CG_DEPTH];
#pragma unroll
            for (uint32_t j = 0; j < CG_DEPTH; ++j) {
                const uint64_t o = o0 + (uint64_t)j * CG_LANES + gl;
                in[j] = o < b8 / 8;
                v[j] = in[j] ? q[o] : uint4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (uint32_t j = 0; j < CG_DEPTH; ++j)
                if (in[j]) {
                    atomicAdd(&tab[v[j].x & 0xFFFFu], 1u); atomicAdd(&tab[v[j].x >> 16], 1u);
                    atomicAdd(&tab[v[j].y & 0xFFFFu], 1u); atomicAdd(&tab[v[j].y >> 16], 1u);
                    atomicAdd(&tab[v[j].z & 0xFFFFu], 1u); atomicAdd(&tab[v[j].z >> 16], 1u);
                    atomicAdd(&tab[v[j].w & 0xFFFFu], 1u); atomicAdd(&tab[v[j].w >> 16], 1u);
                }
        }
        if (head != 0xFFFFu) atomicAdd(&tab[head], 1u);   // (16-bit keys are < BIN_SLOTS: 0xFFFF is no key)
        if (tail != 0xFFFFu) atomicAdd(&tab[tail], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nslots; i += CS_BLOCK) {
        const uint32_t c = tab[i];
        if (c) atomicAdd(counts + slot0 + i, (unsigned long long)c);   // (launches on several streams may count into one table)
    }
}

// a table of one bin: straight over the raw streams (32-bit keys, padding skipped); workgroup `blockIdx.x` of `gridDim.x` takes its share
__global__ __launch_bounds__(CS_BLOCK) void pa_keys_count_raw_kernel(const uint32_t* __restrict__ src, const KeyTops keys_top, unsigned long long* __restrict__ counts,
                                                                     uint64_t counts_len) {
    extern __shared__ uint32_t tab[];   // counts_len counters
    for (uint32_t i = threadIdx.x; i < counts_len; i += CS_BLOCK) tab[i] = 0;
    __syncthreads();
    const uint64_t n4 = stream_len(keys_top) / 4;
    const uint64_t a = n4 * blockIdx.x / gridDim.x, b = n4 * (blockIdx.x + 1) / gridDim.x;
    const uint4* q = reinterpret_cast<const uint4*>(src);
    for (uint64_t i = a + threadIdx.x; i < b; i += CS_BLOCK) {
        const uint4 v = q[i];
        if (v.x != NO_KEY) atomicAdd(&tab[v.x], 1u);
        if (v.y != NO_KEY) atomicAdd(&tab[v.y], 1u);
        if (v.z != NO_KEY) atomicAdd(&tab[v.z], 1u);
        if (v.w != NO_KEY) atomicAdd(&tab[v.w], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < counts_len; i += CS_BLOCK) {
        const uint32_t c = tab[i];
        if (c) atomicAdd(counts + i, (unsigned long long)c);
    }
}

// tables beyond MAX_BINS bins: plain atomics per key
__global__ __launch_bounds__(256) void pa_keys_count_direct_kernel(const uint32_t* __restrict__ keys, const KeyTops keys_top, unsigned long long* __restrict__ counts) {
    const uint64_t n = stream_len(keys_top);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k = keys[i];
        if (k != NO_KEY) atomicAdd(counts + k, 1ull);
    }
}


}  // namespace
// leaves one chunk partly used at its exit
uint64_t key_stream_capacity(uint64_t n_reads, uint32_t nwaves) {   // chunks are filled to the last entry; every wave leaves one partly used (padded)
    return (n_reads / PA_KEY_CHUNK + nwaves + 2) * PA_KEY_CHUNK;
}

static uint64_t nbins_of(uint64_t counts_len) { return (counts_len + BIN_SLOTS - 1) >> PA_KEY_BIN_SHIFT; }

// plain atomics per key: tables beyond MAX_BINS bins — and SMALL batches of a multi-bin table, where three kernels over a few
// thousand keys cost more than the atomics they avoid (one launch instead of three; every small-batch test runs this kernel)
static bool count_direct(uint64_t nbins, uint64_t n_reads) { return nbins > MAX_BINS || (nbins > 1 && n_reads <= PA_COUNT_DIRECT_MAX_READS); }

bool count_keys_partitioned(uint64_t counts_len, uint64_t n_reads) {
    const uint64_t nbins = nbins_of(counts_len);
    return nbins > 1 && !count_direct(nbins, n_reads);
}

static uint32_t tile_capacity(uint64_t keys_cap, uint64_t extra_cap) {
    return (uint32_t)((keys_cap + PT_TILE - 1) / PT_TILE + (extra_cap + PT_TILE - 1) / PT_TILE);
}

void count_keys_scratch(uint64_t counts_len, uint64_t n_reads, uint64_t keys_cap, uint64_t extra_cap, size_t* sorted_bytes, size_t* ctl_bytes) {
    *sorted_bytes = *ctl_bytes = 0;
    if (!count_keys_partitioned(counts_len, n_reads)) return;
    const uint64_t tcap = tile_capacity(keys_cap, extra_cap);
    *sorted_bytes = tcap * PT_TILE * sizeof(uint16_t);
    *ctl_bytes = (nbins_of(counts_len) + 1) * tcap * sizeof(uint32_t);   // run_off
}

int launch_count_keys(const uint32_t* keys, const unsigned long long* keys_top_ptr, uint64_t keys_cap, const unsigned long long* extra_top, uint64_t extra_cap,
                      uint32_t* sorted, uint32_t* ctl, unsigned long long* counts, uint64_t counts_len, int num_cus, hipStream_t stream, uint64_t n_reads,
                      uint32_t pass) {
    if (counts_len == 0) return 0;
    const KeyTops keys_top{keys_top_ptr, keys_cap, extra_top, extra_cap};
    const uint64_t nbins = nbins_of(counts_len);
    const uint32_t cus = num_cus > 0 ? (uint32_t)num_cus : 256u;
    const bool partitioned = count_keys_partitioned(counts_len, n_reads);
    if (pass == 0) {   // what needs only the map kernel's keys: the partition of its chunks (the other paths read the whole stream after resolve)
        if (!partitioned) return 0;
        const uint32_t tcap = tile_capacity(keys_cap, extra_cap);
        const uint32_t G = std::max<uint32_t>(1u, std::min<uint32_t>(cus * 4, (uint32_t)((keys_cap + PT_TILE - 1) / PT_TILE)));
        hipLaunchKernelGGL(pa_keys_part_kernel, dim3(G), dim3(PT_BLOCK), 0, stream, keys, keys_top, 0u, (uint32_t)nbins, tcap, reinterpret_cast<uint16_t*>(sorted), ctl);
        return (int)hipGetLastError();
    }
    const size_t lds = (size_t)(counts_len < BIN_SLOTS ? counts_len : BIN_SLOTS) * 4;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pa_keys_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pa_keys_count_raw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (count_direct(nbins, n_reads)) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)cus * 8, (keys_cap + extra_cap + 255) / 256 + 1);
        hipLaunchKernelGGL(pa_keys_count_direct_kernel, dim3(blocks), dim3(256), 0, stream, keys, keys_top, counts);
        return (int)hipGetLastError();
    }
    if (nbins == 1) {
        hipLaunchKernelGGL(pa_keys_count_raw_kernel, dim3(cus), dim3(CS_BLOCK), lds, stream, keys, keys_top, counts, counts_len);
        return (int)hipGetLastError();
    }
    // the deferred reads' keys: the tiles behind those of pass 0 (3.5 M keys at config 3: a few hundred tiles)
    const uint32_t tcap = tile_capacity(keys_cap, extra_cap);
    const uint32_t G1 = std::max<uint32_t>(1u, std::min<uint32_t>(cus * 4, (uint32_t)((extra_cap + PT_TILE - 1) / PT_TILE)));
    hipLaunchKernelGGL(pa_keys_part_kernel, dim3(G1), dim3(PT_BLOCK), 0, stream, keys, keys_top, 1u, (uint32_t)nbins, tcap, reinterpret_cast<uint16_t*>(sorted), ctl);
    // one workgroup per CU at most (an LDS table of 128 KiB each) and ONE round of them: 270 workgroups on 256 CUs take as long as 512
    uint32_t parts = std::max<uint32_t>(1u, (uint32_t)(cus / nbins));
    parts = std::max<uint32_t>(1u, (uint32_t)knob_int("PA_COUNT_PARTS", (int)parts));   // (A/B knob; never zero: the count kernel divides by it)
    hipLaunchKernelGGL(pa_keys_count_kernel, dim3((uint32_t)nbins * parts), dim3(CS_BLOCK), lds, stream, reinterpret_cast<const uint16_t*>(sorted), (const uint32_t*)ctl, tcap,
                       keys_top, parts, counts, counts_len);
    return (int)hipGetLastError();
}

}  // namespace pa
