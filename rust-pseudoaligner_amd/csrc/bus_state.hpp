// The BUS writer (pa_bus) as csrc/bus.hip builds it, with the kernels of the "collapse" of sorted keys and of the whole records: shared
// with csrc/bus_correct.hip, which rewrites a finished writer's records where they lie. Included by .hip sources only.
#pragma once
#include <hip/hip_runtime.h>

#include <unordered_map>
#include <vector>

#include "bus_host.hpp"
#include "hip_buffer.hpp"
#include "pa_common.hpp"

namespace {   // (kernels and helpers of the including source: every code object gets its own)

using pa::u128;
typedef unsigned long long ull;
constexpr uint32_t BUS_BLOCK = 256;               // 4 waves
enum : uint32_t { BS_READS = 0, BS_R1_SHORT, BS_BARCODE_N, BS_UMI_N, BS_UNMAPPED, BS_BAD_CLASS, BS_RECORDED, BS_RECORDS };

__host__ __device__ inline ull bus_low_mask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }
__device__ inline ull key_lo(u128 k) { return (ull)k; }
__device__ inline ull key_hi(u128 k) { return (ull)(k >> 64); }

// ---- collapse of sorted keys: flag the first of every run, scan, scatter ----
template <class K>
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_heads_kernel(const K* __restrict__ keys, uint32_t n, uint32_t* __restrict__ heads) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i < n) heads[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
// pos = inclusive scan of heads: run r = pos[i] - 1 begins at its head i; start[runs] = n
template <class K>
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_scatter_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ heads, const uint32_t* __restrict__ pos,
                                                                    uint32_t n, K* __restrict__ unique, uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (heads[i]) {
        unique[pos[i] - 1] = keys[i];
        start[pos[i] - 1] = i;
    }
    if (i == n - 1) start[pos[i]] = n;
}
// reads of every run: its length, or the sum of its members' counts (in 64 bits, clamped at 2^32 - 1)
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_run_counts_kernel(const uint32_t* __restrict__ start, uint32_t runs, const uint32_t* __restrict__ counts_in,
                                                                       uint32_t* __restrict__ counts) {
    const uint32_t r = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (r >= runs) return;
    const uint32_t a = start[r], b = start[r + 1];
    if (!counts_in) { counts[r] = b - a; return; }
    ull sum = 0;
    for (uint32_t j = a; j < b; ++j) sum += counts_in[j];
    counts[r] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
}

// whole records: 32 bytes as two 16-byte stores
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_records_kernel(const u128* __restrict__ keys, const uint32_t* __restrict__ counts, uint32_t n, uint32_t umi_bits,
                                                                    pa_bus_record* __restrict__ out) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u128 k = keys[i];
    const ull w = key_hi(k), bc = w >> umi_bits, umi = w & bus_low_mask(umi_bits);
    uint4* o = reinterpret_cast<uint4*>(out + i);
    o[0] = make_uint4((uint32_t)bc, (uint32_t)(bc >> 32), (uint32_t)umi, (uint32_t)(umi >> 32));
    o[1] = make_uint4((uint32_t)key_lo(k), counts[i], 0u, 0u);
}

}  // namespace

struct pa_bus {
    int device = 0;
    uint32_t bc_len = 0, umi_len = 0, num_classes = 0, num_tx = 0;
    const pa_host_index* host = nullptr;
    pa::DeviceBuffer<uint32_t> d_class_ec;
    pa::DeviceBuffer<ull> d_stats, d_err;
    // (key, reads) entries of every batch so far, unsorted across batches
    pa::DeviceBuffer<u128> acc_keys;
    pa::DeviceBuffer<uint32_t> acc_counts;
    uint64_t acc_n = 0;
    // scratch of a batch, kept between batches
    pa::DeviceBuffer<u128> keys, sorted;
    pa::DeviceBuffer<uint32_t> vals, svals, heads, pos, start, which, lread, lread_s, d_n, pool_ids;
    pa::DeviceBuffer<ull> lhash, lhash_s, lhash_u, lens, loff;
    pa::DeviceBuffer<uint8_t> tmp;
    // one list per distinct hash of the run, on the host: list l = list_ids[list_off[l] .. list_off[l + 1])
    std::unordered_map<ull, uint64_t> list_of_hash;
    std::vector<ull> list_hash;
    std::vector<uint64_t> list_off{0};
    std::vector<uint32_t> list_ids;
    bool finished = false;
    uint64_t stats[PA_BUS_STATS] = {};
    pa::DeviceBuffer<pa_bus_record> d_records;   // the records after finish: they stay in HBM until they are asked for or written
    uint64_t n_records = 0;
    pa::bus::EcTable table;
    uint32_t key_bits() const { return 64 + 2 * (bc_len + umi_len); }
};
