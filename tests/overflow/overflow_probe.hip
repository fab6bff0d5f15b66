// Test-only probe of the overflow table of novel classes (tests/test_gpu_overflow_edges.py; never linked into the product). This translation unit
// INCLUDES csrc/collective.hip, so struct pa_overflow, the two kernels and the whole C ABI of the table (pa_overflow_*, pa_comm_*) are the
// product's own text compiled with the product's flags; the rest of the host runtime (pa::fail, pa_counts_len ...) comes from the product
// library the probe is linked against. The probe is linked -Bsymbolic: the table functions it calls, and the ones a test reaches through it,
// are the copies in here, whatever else the process has loaded.
//
// Every export takes host arrays, works on ONE stream (the caller's, or the null stream), synchronises it and returns a pa_status; a HIP
// error comes back as PA_ERR_HIP with HIP's message in pa_last_error().
#include "collective.hip"

namespace {

__global__ void ovp_hash_kernel(const uint32_t* arena, const uint32_t* list, uint64_t n, unsigned long long* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = list_hash_dev(arena + list[2 * i], list[2 * i + 1]);
}

__global__ void ovp_or_kernel(unsigned long long* word, unsigned long long value) { atomicOr(word, value); }

// every {offset, length} entry must lie inside the arena: nothing a test hands over can make a kernel read out of bounds
int lists_in_bounds(const uint32_t* list, uint64_t n, uint64_t arena_words) {
    for (uint64_t i = 0; i < n; ++i)
        if ((uint64_t)list[2 * i] + list[2 * i + 1] > arena_words) return fail(PA_ERR_INVALID_ARG, "list %llu runs past the arena", (unsigned long long)i);
    return PA_OK;
}

}  // namespace

extern "C" {

int ovp_stream_new(void** out) {
    hipStream_t s = nullptr;
    PA_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return PA_OK;
}

int ovp_stream_free(void* s) {
    PA_HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(s)));
    return PA_OK;
}

// What a map launch does with its novel list: `list` ({arena offset, length} x list_entries) and the counter value `ctr` go to the device and
// pa::overflow_after_map files min(ctr, novel_cap) of them. list_entries >= min(ctr, novel_cap) is required, and every entry — those beyond
// the bound too — must lie in the arena.
int ovp_insert(pa_overflow* o, const uint32_t* arena, uint64_t arena_words, const uint32_t* list, uint64_t list_entries, uint64_t ctr, uint64_t novel_cap,
               void* stream) {
    if (!o || !arena || !list || arena_words == 0 || list_entries == 0) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (list_entries < std::min(ctr, novel_cap)) return fail(PA_ERR_INVALID_ARG, "the list is shorter than what the kernel would read");
    if (const int e = lists_in_bounds(list, list_entries, arena_words)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PA_HIP_TRY(hipSetDevice(overflow_device(o)));
    DeviceBuffer<uint32_t> d_arena, d_list;
    DeviceBuffer<unsigned long long> d_ctr;
    if (const int e = d_arena.alloc(arena_words)) return e;
    if (const int e = d_list.alloc(2 * list_entries)) return e;
    if (const int e = d_ctr.alloc(1)) return e;
    const unsigned long long c = ctr;
    PA_HIP_TRY(hipMemcpyAsync(d_arena.get(), arena, arena_words * 4, hipMemcpyHostToDevice, st));
    PA_HIP_TRY(hipMemcpyAsync(d_list.get(), list, list_entries * 8, hipMemcpyHostToDevice, st));
    PA_HIP_TRY(hipMemcpyAsync(d_ctr.get(), &c, 8, hipMemcpyHostToDevice, st));
    const int rc = overflow_after_map(o, d_list.get(), d_ctr.get(), novel_cap, d_arena.get(), st);
    PA_HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

// sizes of the table; then (any of them may be NULL) keys[cap], meta[6 cap], ctl[4]
int ovp_dump(pa_overflow* o, uint64_t* cap, uint64_t* pool_cap, unsigned long long* keys, uint32_t* meta, unsigned long long* ctl) {
    if (!o) return fail(PA_ERR_INVALID_ARG, "null argument");
    PA_HIP_TRY(hipSetDevice(o->device));
    if (cap) *cap = o->cap;
    if (pool_cap) *pool_cap = o->pool_cap;
    if (keys) PA_HIP_TRY(hipMemcpy(keys, o->d_keys.get(), o->cap * 8, hipMemcpyDeviceToHost));
    if (meta) PA_HIP_TRY(hipMemcpy(meta, o->d_meta.get(), o->cap * OVF_META_WORDS * 4, hipMemcpyDeviceToHost));
    if (ctl) PA_HIP_TRY(hipMemcpy(ctl, o->d_ctl.get(), 32, hipMemcpyDeviceToHost));
    return PA_OK;
}

// the 64-bit count of the entry in `slot` (which must hold one)
int ovp_poke_count(pa_overflow* o, uint64_t slot, uint64_t count) {
    if (!o || slot >= o->cap) return fail(PA_ERR_INVALID_ARG, "no such slot");
    PA_HIP_TRY(hipSetDevice(o->device));
    const uint32_t w[2] = {(uint32_t)count, (uint32_t)(count >> 32)};
    PA_HIP_TRY(hipMemcpy(o->d_meta.get() + slot * OVF_META_WORDS + 2, w, 8, hipMemcpyHostToDevice));
    return PA_OK;
}

// ORs `value` into the status word, through the pointer a map launch gets for it (pa::overflow_launch_params)
int ovp_or_status(pa_overflow* o, uint64_t value, void* stream) {
    if (!o) return fail(PA_ERR_INVALID_ARG, "null argument");
    PA_HIP_TRY(hipSetDevice(o->device));
    MapParams p{};
    overflow_launch_params(o, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ovp_or_kernel, dim3(1), dim3(1), 0, st, p.novel_status, (unsigned long long)value);
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipStreamSynchronize(st));
    return PA_OK;
}

// out[i] = pa::list_hash_dev of list i ({arena offset, length} x n)
int ovp_hash(const uint32_t* arena, uint64_t arena_words, const uint32_t* list, uint64_t n, unsigned long long* out, void* stream) {
    if (!arena || !list || !out || arena_words == 0 || n == 0) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (const int e = lists_in_bounds(list, n, arena_words)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DeviceBuffer<uint32_t> d_arena, d_list;
    DeviceBuffer<unsigned long long> d_out;
    if (const int e = d_arena.alloc(arena_words)) return e;
    if (const int e = d_list.alloc(2 * n)) return e;
    if (const int e = d_out.alloc(n)) return e;
    PA_HIP_TRY(hipMemcpyAsync(d_arena.get(), arena, arena_words * 4, hipMemcpyHostToDevice, st));
    PA_HIP_TRY(hipMemcpyAsync(d_list.get(), list, n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ovp_hash_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_arena.get(), d_list.get(), n, d_out.get());
    PA_HIP_TRY(hipGetLastError());
    PA_HIP_TRY(hipMemcpyAsync(out, d_out.get(), n * 8, hipMemcpyDeviceToHost, st));
    PA_HIP_TRY(hipStreamSynchronize(st));
    return PA_OK;
}

}  // extern "C"
