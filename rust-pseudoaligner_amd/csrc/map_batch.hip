// The host-buffer convenience path: reads in host memory -> H2D, encode, map on the null stream (regrow on arena overflow), D2H, classes as CSR in
// read order. One batch at a time per index (pa_index::hmu), on the index's b_* buffers and the launch context of the null stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_index.hpp"

using namespace pa;

namespace pa {
// (pa_common.hpp) the one expansion behind pa_map_batch and pa_map_pairs
void classes_to_csr(const pa_index* idx, pa_read_result* results, uint64_t n, const uint32_t* h_arena, std::vector<uint32_t>& ids, uint64_t* class_offsets,
                    const uint32_t** class_ids) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += results[i].class_len;
    ids.resize(total + 1);
    uint64_t o = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (class_offsets) class_offsets[i] = o;
        if (results[i].class_len) {
            const uint32_t* src = (results[i].class_off & PA_CLASS_REF)
                                      ? idx->h_ec.data() + 4ull * idx->h_class_ref[results[i].class_off & ~PA_CLASS_REF] + 1
                                      : h_arena + results[i].class_off;
            memcpy(ids.data() + o, src, results[i].class_len * 4ull);
        }
        results[i].class_off = (uint32_t)o;
        o += results[i].class_len;
    }
    if (class_offsets) class_offsets[n] = o;
    if (class_ids) *class_ids = ids.data();
}
}  // namespace pa

// The reads of a host batch: ASCII (concatenated, offsets[n+1]) or already 2-bit packed (what a DnaString holds, :450: every
// read starts on a word boundary of `words`, word_offsets[n+1] in words, lens[n] in bases; layout 0 = this library's
// LSB-first words, 1 = MSB-first words: base j in bits 62 - 2 (j % 32)).
struct HostReads {
    const uint8_t* ascii = nullptr;
    const uint64_t* offsets = nullptr;
    const uint64_t* words = nullptr;
    const uint64_t* word_offsets = nullptr;
    const uint32_t* lens = nullptr;
    int layout = 0;
};

static inline uint64_t msb_to_lsb_first(uint64_t w) {   // reverse the order of the 32 two-bit fields
    w = ((w >> 2) & 0x3333333333333333ull) | ((w & 0x3333333333333333ull) << 2);
    w = ((w >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((w & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(w);
}

static int map_batch_host(pa_index* idx, const HostReads& in, uint64_t n, uint32_t allowed,
                          pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids, uint32_t* nodes_flat,
                          uint32_t nodes_stride_cap, uint32_t* nodes_len) {
    const bool packed = in.words != nullptr || in.word_offsets != nullptr;
    if (!idx || !results) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (packed ? (!in.word_offsets || !in.lens || (n && !in.words && in.word_offsets[n] != in.word_offsets[0])) : (!in.offsets || (n && !in.ascii)))
        return fail(PA_ERR_INVALID_ARG, "null argument");
    if (packed && in.layout != 0 && in.layout != 1) return fail(PA_ERR_INVALID_ARG, "packed layout %d (0 = LSB-first, 1 = MSB-first words)", in.layout);
    std::lock_guard<std::mutex> hg(idx->hmu);
    hipStream_t st = nullptr;
    StreamCtx s;   // held across the whole call: a concurrent pa_map_batch_device on the null stream does not interleave with it
    int rc = s.open(idx, st);
    if (rc != PA_OK) return rc;
    uint64_t maxlen = 1;
    for (uint64_t i = 0; i < n; ++i) {
        if (packed) {
            if (in.word_offsets[i + 1] < in.word_offsets[i] || (uint64_t)(in.lens[i] + 31) / 32 > in.word_offsets[i + 1] - in.word_offsets[i])
                return fail(PA_ERR_INVALID_ARG, "read %llu: %u bases do not fit its words", (unsigned long long)i, in.lens[i]);
            maxlen = std::max<uint64_t>(maxlen, in.lens[i]);
        } else {
            if (in.offsets[i + 1] < in.offsets[i]) return fail(PA_ERR_INVALID_ARG, "offsets not monotone at read %llu", (unsigned long long)i);
            maxlen = std::max<uint64_t>(maxlen, in.offsets[i + 1] - in.offsets[i]);
        }
    }
    if (maxlen > PA_MAX_READ_LEN) return fail(PA_ERR_UNSUPPORTED, "read longer than %u bases", PA_MAX_READ_LEN);
    const uint32_t wpr = pa_words_per_read((uint32_t)maxlen);
    if ((rc = grow(idx->b_tiles, pa_tiles_words(n, wpr) + 1)) || (rc = grow(idx->b_lens, n + 64)) || (rc = grow(idx->b_results, n + 1))) return rc;
    if (n == 0) { if (class_offsets) class_offsets[0] = 0; if (class_ids) *class_ids = nullptr; return PA_OK; }
    if (packed) {   // the words go into the tile layout on the host (bases beyond a read's length cleared, as the encoder leaves them)
        std::vector<uint64_t> tiles(pa_tiles_words(n, wpr), 0);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t* w = in.words + in.word_offsets[i];
            const uint32_t len = in.lens[i], nw = (len + 31) / 32;
            uint64_t* dst = tiles.data() + ((i >> 6) * wpr) * 64 + (i & 63);
            for (uint32_t j = 0; j < nw; ++j) {
                uint64_t v = in.layout == 1 ? msb_to_lsb_first(w[j]) : w[j];
                const uint32_t rem = len - 32 * j;
                if (rem < 32) v &= (1ull << (2 * rem)) - 1;
                dst[(uint64_t)j * 64] = v;
            }
        }
        PA_HIP_TRY(hipMemcpyAsync(idx->b_tiles.get(), tiles.data(), tiles.size() * 8, hipMemcpyHostToDevice, st));
        PA_HIP_TRY(hipMemcpyAsync(idx->b_lens.get(), in.lens, n * 4, hipMemcpyHostToDevice, st));
        PA_HIP_TRY(hipStreamSynchronize(st));   // (`tiles` is pageable and dies with this block)
    } else {
        const uint64_t total_ascii = in.offsets[n] - in.offsets[0];
        if ((rc = grow(idx->b_ascii, total_ascii + 64)) || (rc = grow(idx->b_offsets, n + 1))) return rc;
        std::vector<uint64_t> rel(n + 1);
        for (uint64_t i = 0; i <= n; ++i) rel[i] = in.offsets[i] - in.offsets[0];
        PA_HIP_TRY(hipMemcpyAsync(idx->b_ascii.get(), in.ascii + in.offsets[0], total_ascii, hipMemcpyHostToDevice, st));
        PA_HIP_TRY(hipMemcpyAsync(idx->b_offsets.get(), rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        int e = launch_encode(idx->b_ascii.get(), idx->b_offsets.get(), n, wpr, idx->b_tiles.get(), idx->b_lens.get(), st);
        if (e) return fail(PA_ERR_HIP, "encode launch: %s", hipGetErrorString((hipError_t)e));
        PA_HIP_TRY(hipStreamSynchronize(st));   // (`rel` is pageable and dies with this block)
    }
    const uint32_t spill_cap = spill_cap_of(wpr);
    MapLaunch m;
    m.tiles = idx->b_tiles.get(); m.lens = idx->b_lens.get(); m.n_reads = n; m.wpr = wpr; m.allowed = allowed; m.results = idx->b_results.get();
    if (nodes_flat) {
        if ((rc = grow(idx->b_nodes, n * spill_cap)) || (rc = grow(idx->b_nodes_len, n))) return rc;
        m.nodes = idx->b_nodes.get();
        m.nodes_len = idx->b_nodes_len.get();
    }
    uint64_t used = 0;
    auto launch = [&](uint64_t cap) {
        m.arena = idx->b_arena.get();
        m.arena_cap = cap;
        return map_launch_locked(idx, s.cx.get(), st, m);
    };
    const uint64_t hint = pa_map_arena_hint(idx, n);
    if ((rc = grow(idx->b_arena, hint)) || (rc = launch(hint))) return rc;
    rc = map_finish_regrow(idx->b_arena, [&](uint64_t* need) { return map_finish_locked(s.cx.get(), st, &used, need); }, [&] { return launch(idx->b_arena.size()); });
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipMemcpy(results, idx->b_results.get(), n * sizeof(pa_read_result), hipMemcpyDeviceToHost));
    idx->h_arena.resize(used + 1);
    if (used) PA_HIP_TRY(hipMemcpy(idx->h_arena.data(), idx->b_arena.get(), used * 4, hipMemcpyDeviceToHost));
    if (class_offsets || class_ids) classes_to_csr(idx, results, n, idx->h_arena.data(), idx->h_class_ids, class_offsets, class_ids);
    if (nodes_flat) {
        std::vector<uint32_t> hn(n * (size_t)spill_cap), hl(n);
        PA_HIP_TRY(hipMemcpy(hn.data(), m.nodes, hn.size() * 4, hipMemcpyDeviceToHost));
        PA_HIP_TRY(hipMemcpy(hl.data(), m.nodes_len, n * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) {
            nodes_len[i] = hl[i];
            const uint32_t kept = std::min(std::min(hl[i], spill_cap), nodes_stride_cap);
            memcpy(nodes_flat + i * nodes_stride_cap, hn.data() + i * spill_cap, kept * 4ull);
        }
    }
    return PA_OK;
}

// the record of a single read, as pa_map_read* hand it to the caller: 1 mapped, 0 not mapped (n, coverage and mismatches are still reported), else a
// pa_status. src[n]: the ids of its class or the nodes of its trace (`what` / `unit` name them in the message), copied into buf[cap] when the read mapped
static int unpack_one(const pa_read_result& r, const uint32_t* src, uint32_t n, const char* what, const char* unit, uint32_t* buf, uint32_t cap, uint32_t* n_out, uint32_t* coverage,
                      uint32_t* mismatches) {
    if (n_out) *n_out = n;
    if (coverage) *coverage = r.coverage;
    if (mismatches) *mismatches = r.mismatches & ~PA_MAPPED_BIT;
    if (!(r.mismatches & PA_MAPPED_BIT)) return 0;
    if (n > cap) return fail(PA_ERR_INVALID_ARG, "%s buffer too small: %u %s", what, n, unit);
    if (n && buf) memcpy(buf, src, n * 4ull);
    return 1;
}

extern "C" {

int pa_map_batch(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads, uint32_t allowed_mismatches,
                 pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    HostReads in;
    in.ascii = ascii;
    in.offsets = offsets;
    if (!offsets) return fail(PA_ERR_INVALID_ARG, "null argument");
    return map_batch_host(idx, in, n_reads, allowed_mismatches, results, class_offsets, class_ids, nullptr, 0, nullptr);
}

int pa_map_batch_packed(pa_index* idx, const uint64_t* words, const uint64_t* word_offsets, const uint32_t* lens, uint64_t n_reads, int layout,
                        uint32_t allowed_mismatches, pa_read_result* results, uint64_t* class_offsets, const uint32_t** class_ids) {
    HostReads in;
    in.words = words;
    in.word_offsets = word_offsets;
    in.lens = lens;
    in.layout = layout;
    if (!word_offsets || !lens) return fail(PA_ERR_INVALID_ARG, "null argument");
    return map_batch_host(idx, in, n_reads, allowed_mismatches, results, class_offsets, class_ids, nullptr, 0, nullptr);
}

// map_read_with_mismatch on a read the caller holds 2-bit packed (a DnaString): no ASCII round trip
int pa_map_read_packed(pa_index* idx, const uint64_t* words, uint32_t len, int layout, uint32_t allowed_mismatches, uint32_t* class_buf,
                       uint32_t class_cap, uint32_t* class_len, uint32_t* coverage, uint32_t* mismatches) {
    const uint64_t word_offsets[2] = {0, (len + 31) / 32};
    pa_read_result r;
    uint64_t co[2];
    const uint32_t* ids = nullptr;
    const int rc = pa_map_batch_packed(idx, words, word_offsets, &len, 1, layout, allowed_mismatches, &r, co, &ids);
    if (rc != PA_OK) return rc;
    return unpack_one(r, ids, r.class_len, "class", "ids", class_buf, class_cap, class_len, coverage, mismatches);
}

int pa_map_read_with_mismatch(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t allowed_mismatches, uint32_t* class_buf,
                              uint32_t class_cap, uint32_t* class_len, uint32_t* coverage, uint32_t* mismatches) {
    const uint64_t offsets[2] = {0, len};
    pa_read_result r;
    uint64_t co[2];
    const uint32_t* ids = nullptr;
    const int rc = pa_map_batch(idx, ascii, offsets, 1, allowed_mismatches, &r, co, &ids);
    if (rc != PA_OK) return rc;
    return unpack_one(r, ids, r.class_len, "class", "ids", class_buf, class_cap, class_len, coverage, mismatches);
}

int pa_map_read(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t* class_buf, uint32_t class_cap, uint32_t* class_len,
                uint32_t* coverage) {
    return pa_map_read_with_mismatch(idx, ascii, len, PA_DEFAULT_ALLOWED_MISMATCHES, class_buf, class_cap, class_len, coverage, nullptr);
}

int pa_map_read_to_nodes(pa_index* idx, const uint8_t* ascii, uint32_t len, uint32_t allowed_mismatches, uint32_t* node_buf,
                         uint32_t node_cap, uint32_t* num_nodes, uint32_t* coverage, uint32_t* mismatches) {
    const uint64_t offsets[2] = {0, len};
    pa_read_result r;
    uint32_t nn = 0;
    std::vector<uint32_t> tmp(node_cap ? node_cap : 1);
    HostReads in;
    in.ascii = ascii;
    in.offsets = offsets;
    const int rc = map_batch_host(idx, in, 1, allowed_mismatches, &r, nullptr, nullptr, tmp.data(), node_cap, &nn);
    if (rc != PA_OK) return rc;
    return unpack_one(r, tmp.data(), nn, "node", "nodes", node_buf, node_cap, num_nodes, coverage, mismatches);
}

// batch variant of the node trace (test surface)
int pa_map_batch_nodes(pa_index* idx, const uint8_t* ascii, const uint64_t* offsets, uint64_t n_reads, uint32_t allowed_mismatches,
                       pa_read_result* results, uint32_t* nodes_flat, uint32_t nodes_stride, uint32_t* nodes_len) {
    HostReads in;
    in.ascii = ascii;
    in.offsets = offsets;
    if (!offsets) return fail(PA_ERR_INVALID_ARG, "null argument");
    return map_batch_host(idx, in, n_reads, allowed_mismatches, results, nullptr, nullptr, nodes_flat, nodes_stride, nodes_len);
}

}  // extern "C"
