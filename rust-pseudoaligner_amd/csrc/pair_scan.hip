// The pair scan of the paired-FASTQ drivers on the GPU: record i of an R1 window against record i of an R2 window (rec = {id offset, id
// length, sequence offset, length} as fastq_scan.hip leaves them, or as a caller wrote them), and the gather of R2's sequence and R1's
// prefix out of the two window texts into the back-to-back bytes + offsets that pa_encode_reads_device, pa_cell_counter_add_device and
// pa_bus_add_device take. One call handles a SEGMENT: m pairs that land at positions [base, base + m) of a batch.
//
//   pa_pair_ctl_reset_kernel   base == 0 opens a batch: the control block {first bad, max_len1, max_len2, bytes1, bytes2, first outside}
//   pa_pair_match              one lane per pair: rows that point outside their text are refused (nothing of them is read), a trailing "/1" or
//                              "/2" is cut from both ids, lengths and bytes compared, len1 = min(seq_len1, prefix) and len2 = seq_len2
//                              written, pieces longer than LONG_PIECE listed; per wave one reduce and at most one atomic per control word
//   rocPRIM exclusive scan     x 2: the segment's own offsets (u64) of both mates; entry m is the segment's bytes
//   pa_pair_gather             eight lanes per pair: both pieces of the pair, up to LONG_PIECE bytes each, to bytes + running base + offset;
//                              the batch's offsets are written here
//   pa_pair_gather_long        one wave per listed piece (a read of up to PA_MAX_READ_LEN bytes), grid-stride over the list
//   pa_pair_close_kernel       the running bases move on: ctl.bytes += the segment's bytes, off[base + m] = ctl.bytes
//
// The running bases live in the control block, on the device: a segment is scanned and gathered as soon as its two windows are known, so a
// window can be given up behind its last segment's gather and not only when the batch closes, and the host reads the block once per batch.
// A piece is copied in 16-byte stores at 16-byte aligned destinations (its first and last few bytes one by one); the loads are 16 bytes wide
// where source and destination are congruent mod 16, 4 bytes wide where they are congruent mod 4, single bytes otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_prims.hpp"
#include "pa_common.hpp"

namespace pa {
namespace {

constexpr uint32_t LONG_PIECE = 1024;       // bytes beyond which a piece takes a wave of its own
constexpr uint32_t PAIR_LANES = 8;          // lanes that share a pair in pa_pair_gather
constexpr uint32_t LONG_BLOCKS = 2048;      // one-wave blocks of pa_pair_gather_long at most
constexpr uint64_t MAX_SEGMENT = 1ull << 30;
constexpr uint32_t NONE32 = 0xFFFFFFFFu;
enum { CTL_BAD = 0, CTL_MAX1 = 1, CTL_MAX2 = 2, CTL_BYTES1 = 3, CTL_BYTES2 = 4, CTL_OUTSIDE = 5 };

struct Scratch {   // carved out of the caller's block, every part 256-byte aligned
    size_t n_long, len1, len2, loc1, loc2, list, tmp, tmp_bytes, total;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

Scratch scratch_layout(uint64_t m) {
    Scratch s;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    s.n_long = take(4);
    s.len1 = take((m + 1) * 4);
    s.len2 = take((m + 1) * 4);
    s.loc1 = take((m + 1) * 8);
    s.loc2 = take((m + 1) * 8);
    s.list = take(2 * m * 4 + 4);
    s.tmp_bytes = prim_bytes([&](void* t, size_t& b) { return scan_exclusive_on(t, b, (const uint32_t*)nullptr, (uint64_t*)nullptr, (size_t)m + 1, nullptr); });
    s.tmp = take(s.tmp_bytes);
    s.total = at;
    return s;
}

// record.id() with a trailing "/1" or "/2" cut (an id of exactly "/1" becomes empty; "/3" stays)
__device__ __forceinline__ uint32_t cut_mate_suffix(const uint8_t* __restrict__ id, uint32_t len) {
    if (len >= 2 && id[len - 2] == '/' && (id[len - 1] == '1' || id[len - 1] == '2')) return len - 2;
    return len;
}

__device__ __forceinline__ bool row_inside(const uint4 q, uint64_t text_bytes) {
    return (uint64_t)q.x + q.y <= text_bytes && (uint64_t)q.z + q.w <= text_bytes;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_down(v, o, 64));
    return v;
}

__global__ __launch_bounds__(64) void pa_pair_ctl_reset_kernel(unsigned long long* __restrict__ ctl) {
    if (threadIdx.x < PA_PAIRS_CTL_WORDS) ctl[threadIdx.x] = (threadIdx.x == CTL_BAD || threadIdx.x == CTL_OUTSIDE) ? ~0ull : 0ull;
}

__global__ __launch_bounds__(256) void pa_pair_match(const uint8_t* __restrict__ text1, uint64_t text1_bytes, const uint4* __restrict__ rec1, const uint8_t* __restrict__ text2,
                                                     uint64_t text2_bytes, const uint4* __restrict__ rec2, uint32_t m, uint32_t prefix, uint64_t base, uint32_t* __restrict__ len1,
                                                     uint32_t* __restrict__ len2, uint32_t* __restrict__ long_list, uint32_t* __restrict__ n_long,
                                                     unsigned long long* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // (the grid covers m + 1 lanes: lane m closes the scans' input)
    uint32_t bad = NONE32, outside = NONE32, l1 = 0, l2 = 0;
    if (i < m) {
        const uint4 q1 = rec1[i], q2 = rec2[i];
        if (row_inside(q1, text1_bytes) && row_inside(q2, text2_bytes)) {
            const uint8_t* const id1 = text1 + q1.x;
            const uint8_t* const id2 = text2 + q2.x;
            const uint32_t n1 = cut_mate_suffix(id1, q1.y), n2 = cut_mate_suffix(id2, q2.y);
            bool same = n1 == n2;
            for (uint32_t j = 0; same && j < n1; ++j) same = id1[j] == id2[j];
            if (!same) bad = i;
            l1 = min(q1.w, prefix);
            l2 = q2.w;
        } else outside = i;
    }
    if (i <= m) { len1[i] = l1; len2[i] = l2; }
    if (l1 > LONG_PIECE) long_list[atomicAdd(n_long, 1u)] = 2u * i;
    if (l2 > LONG_PIECE) long_list[atomicAdd(n_long, 1u)] = 2u * i + 1u;
    bad = wave_min(bad);
    outside = wave_min(outside);
    const uint32_t mx1 = wave_max(l1), mx2 = wave_max(l2);
    if ((threadIdx.x & 63u) == 0) {
        if (bad != NONE32) atomicMin(&ctl[CTL_BAD], (unsigned long long)(base + bad));
        if (outside != NONE32) atomicMin(&ctl[CTL_OUTSIDE], (unsigned long long)(base + outside));
        if (mx1) atomicMax(&ctl[CTL_MAX1], (unsigned long long)mx1);
        if (mx2) atomicMax(&ctl[CTL_MAX2], (unsigned long long)mx2);
    }
}

// len bytes from src to dst by lanes lane, lane + lanes, ...: whole 16-byte stores at aligned destinations, the ends byte by byte
__device__ __forceinline__ void copy_piece(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len, uint32_t lane, uint32_t lanes) {
    const uint32_t head = min(len, (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u));
    const uint32_t chunks = (len - head) >> 4;
    const uint32_t tail_at = head + 16u * chunks;
    uint8_t* const d = dst + head;
    const uint8_t* const s = src + head;
    const uint32_t rel = (uint32_t)((uintptr_t)s & 15u);
    if (rel == 0) {
        for (uint32_t k = lane; k < chunks; k += lanes) reinterpret_cast<uint4*>(d)[k] = reinterpret_cast<const uint4*>(s)[k];
    } else if ((rel & 3u) == 0) {
        for (uint32_t k = lane; k < chunks; k += lanes) {
            const uint32_t* const w = reinterpret_cast<const uint32_t*>(s) + 4u * k;
            reinterpret_cast<uint4*>(d)[k] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (uint32_t k = lane; k < chunks; k += lanes) {
            const uint8_t* const b = s + 16u * k;
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)b[j] << (8u * (j & 3u));
            reinterpret_cast<uint4*>(d)[k] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    for (uint32_t j = lane; j < head; j += lanes) dst[j] = src[j];
    for (uint32_t j = tail_at + lane; j < len; j += lanes) dst[j] = src[j];
}

__global__ __launch_bounds__(256) void pa_pair_gather(const uint8_t* __restrict__ text1, const uint4* __restrict__ rec1, const uint8_t* __restrict__ text2,
                                                      const uint4* __restrict__ rec2, uint32_t m, uint64_t base, const uint32_t* __restrict__ len1,
                                                      const uint32_t* __restrict__ len2, const uint64_t* __restrict__ loc1, const uint64_t* __restrict__ loc2,
                                                      uint8_t* __restrict__ bytes1, uint64_t cap1, uint64_t* __restrict__ off1, uint8_t* __restrict__ bytes2, uint64_t cap2,
                                                      uint64_t* __restrict__ off2, const unsigned long long* __restrict__ ctl) {
    constexpr uint32_t PAIRS = 256 / PAIR_LANES;   // pairs of a block
    const uint64_t run1 = ctl[CTL_BYTES1], run2 = ctl[CTL_BYTES2];   // where the segment begins in the batch's bytes
    if (threadIdx.x < PAIRS) {   // the block's offsets: one coalesced store per mate
        const uint32_t q = blockIdx.x * PAIRS + threadIdx.x;
        if (q < m) { off1[base + q] = run1 + loc1[q]; off2[base + q] = run2 + loc2[q]; }
    }
    const uint32_t p = blockIdx.x * PAIRS + threadIdx.x / PAIR_LANES, sub = threadIdx.x % PAIR_LANES;
    if (p >= m) return;
    const uint32_t l1 = len1[p], l2 = len2[p];
    const uint64_t o1 = run1 + loc1[p], o2 = run2 + loc2[p];
    if (l2 && l2 <= LONG_PIECE && o2 + l2 <= cap2) copy_piece(bytes2 + o2, text2 + rec2[p].z, l2, sub, PAIR_LANES);
    if (l1 && l1 <= LONG_PIECE && o1 + l1 <= cap1) copy_piece(bytes1 + o1, text1 + rec1[p].z, l1, sub, PAIR_LANES);
}

__global__ __launch_bounds__(64) void pa_pair_gather_long(const uint8_t* __restrict__ text1, const uint4* __restrict__ rec1, const uint8_t* __restrict__ text2,
                                                          const uint4* __restrict__ rec2, uint32_t m, const uint32_t* __restrict__ len1, const uint32_t* __restrict__ len2,
                                                          const uint64_t* __restrict__ loc1, const uint64_t* __restrict__ loc2, uint8_t* __restrict__ bytes1, uint64_t cap1,
                                                          uint8_t* __restrict__ bytes2, uint64_t cap2, const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ n_long,
                                                          const unsigned long long* __restrict__ ctl) {
    const uint32_t n = min(*n_long, 2u * m);
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t e = long_list[k], p = e >> 1;
        if (p >= m) continue;
        if (e & 1u) {
            const uint64_t o = ctl[CTL_BYTES2] + loc2[p];
            const uint32_t l = len2[p];
            if (o + l <= cap2) copy_piece(bytes2 + o, text2 + rec2[p].z, l, threadIdx.x, 64);
        } else {
            const uint64_t o = ctl[CTL_BYTES1] + loc1[p];
            const uint32_t l = len1[p];
            if (o + l <= cap1) copy_piece(bytes1 + o, text1 + rec1[p].z, l, threadIdx.x, 64);
        }
    }
}

__global__ __launch_bounds__(64) void pa_pair_close_kernel(uint32_t m, uint64_t base, const uint64_t* __restrict__ loc1, const uint64_t* __restrict__ loc2,
                                                           uint64_t* __restrict__ off1, uint64_t* __restrict__ off2, unsigned long long* __restrict__ ctl) {
    if (threadIdx.x != 0) return;
    const uint64_t b1 = ctl[CTL_BYTES1] + (m ? loc1[m] : 0), b2 = ctl[CTL_BYTES2] + (m ? loc2[m] : 0);
    ctl[CTL_BYTES1] = b1;
    ctl[CTL_BYTES2] = b2;
    off1[base + m] = b1;
    off2[base + m] = b2;
}

}  // namespace

size_t pairs_gather_scratch_bytes(uint64_t m) { return m > MAX_SEGMENT ? 0 : scratch_layout(m).total; }

// one segment, on the current device (no device query, no hipSetDevice): what pa_pairs_gather_device enqueues
int pairs_gather_launch(const uint8_t* d_text1, uint64_t text1_bytes, const uint32_t* d_rec1, const uint8_t* d_text2, uint64_t text2_bytes, const uint32_t* d_rec2, uint64_t m,
                        uint32_t prefix, uint64_t base, uint8_t* d_bytes1, uint64_t cap1, uint64_t* d_off1, uint8_t* d_bytes2, uint64_t cap2, uint64_t* d_off2, uint64_t* d_ctl,
                        void* d_scratch, size_t scratch_bytes, void* stream_) {
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (m > MAX_SEGMENT) return fail(PA_ERR_UNSUPPORTED, "pa_pairs_gather_device: a segment of %llu pairs (at most %llu)", (unsigned long long)m, (unsigned long long)MAX_SEGMENT);
    const Scratch L = scratch_layout(m);
    if (scratch_bytes < L.total) return fail(PA_ERR_BUFFER_TOO_SMALL, "pa_pairs_gather_device: %zu bytes of scratch, pa_pairs_gather_scratch_bytes(%llu) = %zu", scratch_bytes, (unsigned long long)m, L.total);
    uint8_t* const sc = static_cast<uint8_t*>(d_scratch);
    uint32_t* const n_long = reinterpret_cast<uint32_t*>(sc + L.n_long);
    uint32_t* const len1 = reinterpret_cast<uint32_t*>(sc + L.len1);
    uint32_t* const len2 = reinterpret_cast<uint32_t*>(sc + L.len2);
    uint64_t* const loc1 = reinterpret_cast<uint64_t*>(sc + L.loc1);
    uint64_t* const loc2 = reinterpret_cast<uint64_t*>(sc + L.loc2);
    uint32_t* const list = reinterpret_cast<uint32_t*>(sc + L.list);
    unsigned long long* const ctl = reinterpret_cast<unsigned long long*>(d_ctl);
    const uint4* const rec1 = reinterpret_cast<const uint4*>(d_rec1);
    const uint4* const rec2 = reinterpret_cast<const uint4*>(d_rec2);
    hipError_t e = hipSuccess;
    auto launched = [&](const char* what) {
        e = hipGetLastError();
        return e == hipSuccess ? PA_OK : fail(PA_ERR_HIP, "pa_pairs_gather_device: %s: %s", what, hipGetErrorString(e));
    };
    int rc = PA_OK;
    if (base == 0) {
        hipLaunchKernelGGL(pa_pair_ctl_reset_kernel, dim3(1), dim3(64), 0, stream, ctl);
        if ((rc = launched("reset")) != PA_OK) return rc;
    }
    if (m) {
        const uint32_t m32 = (uint32_t)m;
        PA_HIP_TRY(hipMemsetAsync(n_long, 0, 4, stream));
        hipLaunchKernelGGL(pa_pair_match, dim3(grid_for(m + 1)), dim3(256), 0, stream, d_text1, text1_bytes, rec1, d_text2, text2_bytes, rec2, m32, prefix, base, len1, len2, list,
                           n_long, ctl);
        if ((rc = launched("match")) != PA_OK) return rc;
        size_t tb = L.tmp_bytes;
        PA_HIP_TRY(scan_exclusive_on(sc + L.tmp, tb, (const uint32_t*)len1, loc1, (size_t)m + 1, stream));
        tb = L.tmp_bytes;
        PA_HIP_TRY(scan_exclusive_on(sc + L.tmp, tb, (const uint32_t*)len2, loc2, (size_t)m + 1, stream));
        hipLaunchKernelGGL(pa_pair_gather, dim3(grid_for(m, 256 / PAIR_LANES)), dim3(256), 0, stream, d_text1, rec1, d_text2, rec2, m32, base, (const uint32_t*)len1,
                           (const uint32_t*)len2, (const uint64_t*)loc1, (const uint64_t*)loc2, d_bytes1, cap1, d_off1, d_bytes2, cap2, d_off2, (const unsigned long long*)ctl);
        if ((rc = launched("gather")) != PA_OK) return rc;
        const uint32_t long_blocks = (uint32_t)std::min<uint64_t>(2 * m, LONG_BLOCKS);
        hipLaunchKernelGGL(pa_pair_gather_long, dim3(long_blocks), dim3(64), 0, stream, d_text1, rec1, d_text2, rec2, m32, (const uint32_t*)len1, (const uint32_t*)len2,
                           (const uint64_t*)loc1, (const uint64_t*)loc2, d_bytes1, cap1, d_bytes2, cap2, (const uint32_t*)list, (const uint32_t*)n_long,
                           (const unsigned long long*)ctl);
        if ((rc = launched("gather of long reads")) != PA_OK) return rc;
    }
    hipLaunchKernelGGL(pa_pair_close_kernel, dim3(1), dim3(64), 0, stream, (uint32_t)m, base, (const uint64_t*)loc1, (const uint64_t*)loc2, d_off1, d_off2, ctl);
    return launched("close");
}

}  // namespace pa

extern "C" size_t pa_pairs_gather_scratch_bytes(uint64_t m) { return pa::pairs_gather_scratch_bytes(m); }

extern "C" int pa_pairs_gather_device(int device, const uint8_t* d_text1, uint64_t text1_bytes, const uint32_t* d_rec1, const uint8_t* d_text2, uint64_t text2_bytes,
                                      const uint32_t* d_rec2, uint64_t m, uint32_t prefix, uint64_t base, uint8_t* d_bytes1, uint64_t cap1, uint64_t* d_off1, uint8_t* d_bytes2,
                                      uint64_t cap2, uint64_t* d_off2, uint64_t* d_ctl, void* d_scratch, size_t scratch_bytes, void* stream) {
    using namespace pa;
    if (!d_off1 || !d_off2 || !d_ctl || !d_scratch) return fail(PA_ERR_INVALID_ARG, "pa_pairs_gather_device: null argument");
    if (m && (!d_rec1 || !d_rec2 || (text1_bytes && !d_text1) || (text2_bytes && !d_text2) || (cap1 && !d_bytes1) || (cap2 && !d_bytes2)))
        return fail(PA_ERR_INVALID_ARG, "pa_pairs_gather_device: null argument");
    if (((uintptr_t)d_rec1 | (uintptr_t)d_rec2) & 15u) return fail(PA_ERR_INVALID_ARG, "pa_pairs_gather_device: record tables are 16-byte aligned");
    if (((uintptr_t)d_scratch & 255u) || ((uintptr_t)d_ctl & 7u) || (((uintptr_t)d_off1 | (uintptr_t)d_off2) & 7u))
        return fail(PA_ERR_INVALID_ARG, "pa_pairs_gather_device: scratch is 256-byte aligned, offsets and control block 8-byte aligned");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        return fail(PA_ERR_NO_DEVICE, "no HIP device: pairs are matched and gathered on the GPU, there is no CPU fallback");
    }
    if (hipSetDevice(device) != hipSuccess) return fail(PA_ERR_HIP, "hipSetDevice(%d) failed", device);
    return pairs_gather_launch(d_text1, text1_bytes, d_rec1, d_text2, text2_bytes, d_rec2, m, prefix, base, d_bytes1, cap1, d_off1, d_bytes2, cap2, d_off2, d_ctl, d_scratch,
                               scratch_bytes, stream);
}
