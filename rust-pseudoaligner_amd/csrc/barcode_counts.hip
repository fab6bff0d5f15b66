// Per-barcode (single-cell) class counts — SURVEY.md §8f.3, the use the reference was written for (README.md:3: a
// pseudo-alignment tool for single-cell RNA-seq): every read carries the index of its cell barcode, and what downstream wants
// is the SPARSE matrix (barcode, equivalence class) -> reads. On the GPU: one 64-bit key per read (barcode << 32 | column, the
// columns being those of the dense count table: class id, or novel / empty / unmapped), a radix sort of the keys and a
// run-length encode — sorted unique keys with their counts, ready for a CSR / triplet matrix on the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "hip_buffer.hpp"
#include "kernel_utils.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

using namespace pa;

namespace {

__global__ __launch_bounds__(256) void pa_barcode_keys_kernel(const pa_read_result* __restrict__ results, const uint32_t* __restrict__ arena,
                                                              const uint32_t* __restrict__ barcode, uint64_t n_reads, const DevIndexView ix,
                                                              const uint32_t* __restrict__ class_table, uint64_t class_table_size,
                                                              unsigned long long* __restrict__ keys) {
    const uint32_t num_classes = ix.num_classes;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const pa_read_result r = results[i];
    uint32_t col;
    if (!(r.mismatches & PA_MAPPED_BIT)) col = num_classes + 2;
    else if (r.class_len == 0) col = num_classes + 1;
    else {
        uint32_t c = (r.class_off & PA_CLASS_REF) ? (r.class_off & ~PA_CLASS_REF) : class_of_list(arena + r.class_off, r.class_len, ix, class_table, class_table_size);
        col = c == 0xFFFFFFFFu ? num_classes : c;
    }
    keys[i] = ((unsigned long long)barcode[i] << 32) | col;
}

}  // namespace

namespace pa {

// device_index.hip hands over the pieces of the index this needs
int barcode_counts(const DevIndexView& ix, const uint32_t* class_table, uint64_t class_table_size, const pa_read_result* d_results,
                   const uint32_t* d_arena, const uint32_t* d_barcode, uint64_t n, uint32_t barcode_bits, uint64_t* d_keys, uint32_t* d_vals,
                   uint64_t* n_entries, hipStream_t stream) {
    *n_entries = 0;
    if (n == 0) return PA_OK;
    if (n > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "at most 2^31-1 reads per call");
    DeviceBuffer<unsigned long long> keys_in, keys_sorted;
    DeviceBuffer<unsigned int> d_runs;
    DeviceBuffer<uint8_t> tmp;
    int e = keys_in.alloc(n);
    if (e == PA_OK) e = keys_sorted.alloc(n);
    if (e == PA_OK) e = d_runs.alloc(1);
    if (e != PA_OK) return e;
    hipLaunchKernelGGL(pa_barcode_keys_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_results, d_arena, d_barcode, n, ix, class_table,
                       class_table_size, keys_in.get());
    PA_HIP_TRY(hipGetLastError());
    uint32_t col_bits = 1;
    while (col_bits < 32 && (1ull << col_bits) < (uint64_t)ix.num_classes + 3) ++col_bits;
    const int end_bit = (int)(32 + (barcode_bits ? (barcode_bits > 32 ? 32 : barcode_bits) : 32));
    size_t sort_bytes = 0, rle_bytes = 0;
    // only the bits that can differ are sorted: the column's low bits and the barcode's
    PA_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys_in.get(), keys_sorted.get(), (int)n, 0, end_bit, stream));
    PA_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, keys_sorted.get(), (unsigned long long*)d_keys, d_vals, d_runs.get(), (int)n, stream));
    if ((e = tmp.alloc(sort_bytes > rle_bytes ? sort_bytes : rle_bytes)) != PA_OK) return e;
    (void)col_bits;
    PA_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp.get(), sort_bytes, keys_in.get(), keys_sorted.get(), (int)n, 0, end_bit, stream));
    PA_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(tmp.get(), rle_bytes, keys_sorted.get(), (unsigned long long*)d_keys, d_vals, d_runs.get(), (int)n, stream));
    unsigned int runs = 0;
    PA_HIP_TRY(hipMemcpyAsync(&runs, d_runs.get(), 4, hipMemcpyDeviceToHost, stream));
    PA_HIP_TRY(hipStreamSynchronize(stream));
    *n_entries = runs;
    return PA_OK;
}

}  // namespace pa
