// The BUS writer (pa_bus) as csrc/bus.hip builds it, and what the stages over its records (csrc/bus_correct.hip, csrc/bus_knee.hip, csrc/bus_umi.hip) share with it:
// a record as two 16-byte words, the kernel that writes whole records from sorted keys, the sort + collapse tail of a stage that rewrote keys, and the two call frames of a stage, over records from
// the host and over a finished writer's records where they lie. Included by the BUS .hip sources only.
#pragma once
#include <hip/hip_runtime.h>

#include <unordered_map>
#include <vector>

#include "bus_host.hpp"
#include "device_prims.hpp"
#include "hip_buffer.hpp"
#include "pa_common.hpp"

namespace {   // (kernels and helpers of the including source: every code object gets its own)

using pa::u128;
typedef unsigned long long ull;
constexpr uint32_t BUS_BLOCK = 256;               // 4 waves
enum : uint32_t { BS_READS = 0, BS_R1_SHORT, BS_BARCODE_N, BS_UMI_N, BS_UNMAPPED, BS_BAD_CLASS, BS_RECORDED, BS_RECORDS };

__device__ inline ull key_lo(u128 k) { return (ull)k; }
__device__ inline ull key_hi(u128 k) { return (ull)(k >> 64); }

// reads of every run of a collapse (start[runs + 1]): its length, or with counts_in the sum of its members' counts (in 64 bits, clamped at
// 2^32 - 1). The writer's clamp, for bus.hip and bus_correct.hip: not a template, so it cannot stand in device_prims.hpp beside the collapse
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
inline int run_counts(hipStream_t s, const uint32_t* start, uint32_t runs, const uint32_t* counts_in, uint32_t* counts) {
    return pa::launch(pa_bus_run_counts_kernel, pa::grid_for(runs, BUS_BLOCK), BUS_BLOCK, s, start, runs, counts_in, counts);
}

// a record's 32 bytes as two 16-byte words: barcode lo hi, umi lo hi | ec, count, flags, pad
struct RecordWords { uint4 a, c; };
__device__ inline RecordWords load_record(const pa_bus_record* __restrict__ r) {
    const uint4* in = reinterpret_cast<const uint4*>(r);
    return RecordWords{in[0], in[1]};
}
__device__ inline void store_record(pa_bus_record* __restrict__ r, const RecordWords w) {
    uint4* o = reinterpret_cast<uint4*>(r);
    o[0] = w.a;
    o[1] = w.c;
}
__device__ inline void copy_record(pa_bus_record* __restrict__ dst, const pa_bus_record* __restrict__ src) { store_record(dst, load_record(src)); }

// whole records from sorted keys (barcode | UMI) << SHIFT | ec ^ EC_FLIP, the ec in the key's low 32 bits
template <uint32_t SHIFT, uint32_t EC_FLIP>
__global__ __launch_bounds__(BUS_BLOCK) void pa_bus_records_kernel(const u128* __restrict__ keys, const uint32_t* __restrict__ counts, uint32_t n, uint32_t umi_bits,
                                                                    pa_bus_record* __restrict__ out) {
    const uint32_t i = blockIdx.x * BUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u128 k = keys[i];
    const ull w = (ull)(k >> SHIFT), bc = w >> umi_bits, umi = w & pa::low_mask(umi_bits);
    store_record(out + i, RecordWords{make_uint4((uint32_t)bc, (uint32_t)(bc >> 32), (uint32_t)umi, (uint32_t)(umi >> 32)), make_uint4((uint32_t)k ^ EC_FLIP, counts[i], 0u, 0u)});
}

constexpr uint32_t EC_BIAS = 0x80000000u;      // a rewritten key holds ec + 2^31: integer order of the key = (barcode, UMI, ec as int32)

// The tail of a stage that rewrote barcodes or UMIs (bus_correct.hip, bus_umi.hip): keys[n] = (barcode | UMI) << 32 | ec + 2^31 with their counts,
// n >= 1 -> d_out[M] whole records. moved: a key changed, so the keys are sorted over their key_bits live bits and equal ones joined (counts summed
// in 64 bits, clamped); otherwise they are sorted and distinct as they lie. keys and counts are used up
inline int records_from_keys(hipStream_t s, pa::DeviceBuffer<uint8_t>& tmp, pa::DeviceBuffer<u128>& keys, pa::DeviceBuffer<uint32_t>& counts, uint32_t n, bool moved,
                             uint32_t key_bits, uint32_t umi_bits, pa::DeviceBuffer<pa_bus_record>& d_out, uint32_t& M) {
    int e;
    M = n;
    if (moved) {
        pa::DeviceBuffer<u128> k1, k2;
        pa::DeviceBuffer<uint32_t> c1, c2, heads, pos, start;
        if ((e = k1.alloc(n)) || (e = k2.alloc(n)) || (e = c1.alloc(n)) || (e = c2.alloc(n)) || (e = heads.alloc(n)) || (e = pos.alloc(n)) || (e = start.alloc((size_t)n + 1)))
            return e;
        if ((e = pa::sort_pairs(s, tmp, (const u128*)keys.get(), k1.get(), (const uint32_t*)counts.get(), c1.get(), (size_t)n, 0, key_bits))) return e;
        if ((e = pa::collapse_runs(s, tmp, pa::KeyArray<u128>{k1.get()}, n, heads.get(), pos.get(), k2.get(), start.get(), M)) ||
            (e = run_counts(s, start.get(), M, c1.get(), c2.get())))
            return e;
        PA_HIP_TRY(hipStreamSynchronize(s));   // (the scratch of this block is freed at its end)
        keys = std::move(k2);
        counts = std::move(c2);
    }
    if ((e = d_out.alloc(M))) return e;
    return pa::launch(pa_bus_records_kernel<32, EC_BIAS>, pa::grid_for(M, BUS_BLOCK), BUS_BLOCK, s, (const u128*)keys.get(), (const uint32_t*)counts.get(), M, umi_bits, d_out.get());
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

namespace {

// ---- the call frame of a stage over records from the host: behind the stage's own checks of its arguments. stage(d_in, n) runs on the index's
// device with the n >= 1 records uploaded; empty() answers for no records, without device work ----
template <class Stage, class Empty>
int on_host_records(pa_index* idx, const pa_bus_record* in, uint64_t n, Stage&& stage, Empty&& empty) {
    int e;
    if ((e = pa::have_device())) return e;
    if (!idx) return pa::fail(PA_ERR_INVALID_ARG, "null argument");
    if (n == 0) return empty();
    const uint32_t *h_ec = nullptr, *h_ref = nullptr;
    int device = 0;
    pa::index_host_classes(idx, &h_ec, &h_ref, &device);
    PA_HIP_TRY(hipSetDevice(device));
    pa::DeviceBuffer<pa_bus_record> d_in;
    if ((e = pa::upload(d_in, in, (size_t)n))) return e;
    return stage((const pa_bus_record*)d_in.get(), (uint32_t)n);
}
// the n_out records a stage left in d_out -> out[cap], unless out is null
inline int deliver_records(const pa::DeviceBuffer<pa_bus_record>& d_out, uint64_t n_out, pa_bus_record* out, uint64_t cap) {
    if (!out) return PA_OK;
    if (cap < n_out) return pa::fail(PA_ERR_BUFFER_TOO_SMALL, "%llu records, room for %llu", (ull)n_out, (ull)cap);
    if (n_out) PA_HIP_TRY(hipMemcpy(out, d_out.get(), n_out * sizeof(pa_bus_record), hipMemcpyDeviceToHost));
    return PA_OK;
}

// ---- ... and over a finished writer's records where they lie: `unfinished` is the stage's message for a writer before pa_bus_finish, the stage's
// own checks stand between the two ----
inline int finished_writer(const pa_bus* b, const char* unfinished) {
    if (!b) return pa::fail(PA_ERR_INVALID_ARG, "null argument");
    if (!b->finished) return pa::fail(PA_ERR_INVALID_ARG, "%s", unfinished);
    return PA_OK;
}
template <class Stage, class Empty>
int on_writer_records(const pa_bus* b, Stage&& stage, Empty&& empty) {
    if (b->n_records > 0x7FFFFFFFull) return pa::fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 records");
    if (b->n_records == 0) return empty();
    PA_HIP_TRY(hipSetDevice(b->device));
    return stage((const pa_bus_record*)b->d_records.get(), (uint32_t)b->n_records);
}
// ... for a stage that rewrites: the output of stage(d_in, n, d_out, &n_out) takes the place of the writer's records (a failing stage leaves the
// writer as it was)
template <class Stage, class Empty>
int rewrite_writer_records(pa_bus* b, Stage&& stage, Empty&& empty) {
    return on_writer_records(b, [&](const pa_bus_record* d_in, uint32_t n) {
        pa::DeviceBuffer<pa_bus_record> d_out;
        uint64_t n_out = 0;
        const int e = stage(d_in, n, d_out, &n_out);
        if (e != PA_OK) return e;
        b->d_records = std::move(d_out);
        b->n_records = n_out;
        b->stats[BS_RECORDS] = n_out;
        return e;
    }, empty);
}
// the answer of a stage that has nothing to say about no records
inline int empty_ok() { return PA_OK; }

}  // namespace
