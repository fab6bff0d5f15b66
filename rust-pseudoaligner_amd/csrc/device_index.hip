// The device index and the map launch: index create / destroy / stats, the per-stream launch context, launch geometry, the sequencing of the map,
// resolve and count kernels, finish, release and timing, and the C ABI entry points that launch on device buffers.
// There is NO CPU fallback anywhere in this file: without a usable GPU every entry point fails with
// PA_ERR_NO_DEVICE / PA_ERR_HIP and a message in pa_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "device_flatten.hpp"
#include "device_index.hpp"
#include "lane_steps.hpp"

using namespace pa;

namespace {

uint64_t list_hash_host(const uint32_t* v, uint32_t n) {   // must equal list_hash_dev (kernel_utils.hpp)
    uint64_t h = 0x243f6a8885a308d3ull ^ n;
    for (uint32_t i = 0; i < n; ++i) h = mix64(h ^ v[i]) + 0x9e3779b97f4a7c15ull;
    return h;
}

}  // namespace

namespace pa {

void LaunchCtx::release() {
    if (side) (void)hipStreamSynchronize(side);
    ctl.release();
    for (DeviceBuffer<uint32_t>* b : {&spill, &trace, &novel, &keys, &keys_sorted, &keys_ctl, &defer}) b->release();
    for (hipEvent_t e : {ev0, ev1, ev2, ev3, fork, join})
        if (e) (void)hipEventDestroy(e);
    ev0 = ev1 = ev2 = ev3 = fork = join = nullptr;
    if (side) (void)hipStreamDestroy(side);
    side = nullptr;
    timed = false;
}

void* Parked::take(std::mutex& mu) {
    std::lock_guard<std::mutex> g(mu);
    if (held.empty()) return nullptr;
    void* obj = held.back().first;
    held.pop_back();
    return obj;
}
void Parked::put(std::mutex& mu, void* obj, void (*free_fn)(void*)) {
    {
        std::lock_guard<std::mutex> g(mu);
        if (held.size() < cap) {
            held.emplace_back(obj, free_fn);
            return;
        }
    }
    free_fn(obj);
}

void index_host_classes(const pa_index* idx, const uint32_t** ec, const uint32_t** class_ref, int* device) {
    *ec = idx->h_ec.data();
    *class_ref = idx->h_class_ref.data();
    *device = idx->device;
}
void index_pair_view(pa_index* idx, PairIndexView* out) {
    std::lock_guard<std::mutex> g(idx->mu);
    *out = PairIndexView{idx->dv, idx->d_class_table.get(), idx->class_table_size, idx->ovf, idx->device, idx->num_cus};
}
void index_host_class_text(pa_index* idx, const uint64_t** off, const char** text) {
    std::call_once(idx->class_text_once, [idx] {
        const uint32_t nc = idx->stats.num_classes;
        const uint32_t* ec = idx->h_ec.data();
        const uint32_t* cref = idx->h_class_ref.data();
        auto digits = [](uint32_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; ++d; } return d; };
        std::vector<uint64_t>& off_v = idx->h_class_text_off;
        off_v.assign((size_t)nc + 1, 0);
        const int T = std::max(1, std::min(16, usable_threads()));
        const uint32_t* clen = idx->h_class_len.data();
        auto ids_of = [&](uint32_t c, const uint32_t*& ids, uint32_t& n) {   // (the length the flattener noted: nothing is derived from where the next record lies)
            ids = ec + 4ull * cref[c] + 1;
            n = clen[c];
        };
        {
            std::vector<std::thread> th;
            for (int t = 0; t < T; ++t)
                th.emplace_back([&, t] {
                    for (uint64_t c = (uint64_t)nc * t / T; c < (uint64_t)nc * (t + 1) / T; ++c) {
                        const uint32_t* ids; uint32_t n;
                        ids_of((uint32_t)c, ids, n);
                        uint64_t len = n ? 2ull * (n - 1) : 0;
                        for (uint32_t j = 0; j < n; ++j) len += digits(ids[j]);
                        off_v[c + 1] = len;
                    }
                });
            for (auto& x : th) x.join();
        }
        for (uint32_t c = 0; c < nc; ++c) off_v[c + 1] += off_v[c];
        idx->h_class_text.resize(off_v[nc] + 16);
        {
            std::vector<std::thread> th;
            for (int t = 0; t < T; ++t)
                th.emplace_back([&, t] {
                    for (uint64_t c = (uint64_t)nc * t / T; c < (uint64_t)nc * (t + 1) / T; ++c) {
                        const uint32_t* ids; uint32_t n;
                        ids_of((uint32_t)c, ids, n);
                        char* o = idx->h_class_text.data() + off_v[c];
                        for (uint32_t j = 0; j < n; ++j) {
                            if (j) { *o++ = ','; *o++ = ' '; }
                            char b[10]; int k = 10; uint32_t v = ids[j];
                            do { b[--k] = (char)('0' + v % 10); v /= 10; } while (v);
                            memcpy(o, b + k, (size_t)(10 - k)); o += 10 - k;
                        }
                    }
                });
            for (auto& x : th) x.join();
        }
    });
    *off = idx->h_class_text_off.data();
    *text = idx->h_class_text.data();
}
int index_device_class_text(pa_index* idx, const uint64_t** d_off, const uint8_t** d_text) {
    const uint64_t* off = nullptr;
    const char* txt = nullptr;
    index_host_class_text(idx, &off, &txt);
    std::lock_guard<std::mutex> g(idx->mu);
    if (!idx->d_class_text.get()) {   // (d_class_text is uploaded last: it is there only when both are)
        if (hipSetDevice(idx->device) != hipSuccess) return fail(PA_ERR_HIP, "hipSetDevice failed");
        int e = upload(idx->d_class_text_off, off, idx->h_class_text_off.size());
        if (e == PA_OK) e = upload(idx->d_class_text, reinterpret_cast<const uint8_t*>(txt), idx->h_class_text.size());
        if (e != PA_OK) return e;
    }
    *d_off = idx->d_class_text_off.get();
    *d_text = idx->d_class_text.get();
    return PA_OK;
}
void* index_take_ingest_cache(pa_index* idx) { return idx->ingest_caches.take(idx->mu); }
void index_put_ingest_cache(pa_index* idx, void* cache, void (*free_fn)(void*)) { idx->ingest_caches.put(idx->mu, cache, free_fn); }
void* index_take_host_pipe(pa_index* idx) { return idx->host_pipes.take(idx->mu); }
void index_put_host_pipe(pa_index* idx, void* pipe, void (*free_fn)(void*)) { idx->host_pipes.put(idx->mu, pipe, free_fn); }

}  // namespace pa

extern "C" {

void pa_index_destroy(pa_index* idx) {
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    {   // (releases their streams' contexts)
        std::vector<std::pair<void*, void (*)(void*)>> parked;
        { std::lock_guard<std::mutex> g(idx->mu); parked.swap(idx->ingest_caches.held); parked.insert(parked.end(), idx->host_pipes.held.begin(), idx->host_pipes.held.end()); idx->host_pipes.held.clear(); }
        for (auto& c : parked) c.second(c.first);
    }
    for (auto& kv : idx->ctxs) kv.second->release();
    delete idx;   // (the index's own buffers, with its device current)
}

int pa_index_create(const pa_flat_index* flat, int device, pa_index** out) {
    if (!flat || !out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int rc = use_device(device);
    if (rc != PA_OK) return rc;
    FlatDevice fd;
    int threads = usable_threads();
    if (threads < 1) threads = 1;
    // classes, window table, edges, chains and their blocks on the host; the dictionary (6.6 GB at config 3) is built on the GPU
    // from the uploaded blocks (index_fill.hip) — nothing of the table exists on the host or crosses PCIe
    rc = flatten_for_device(*flat, threads, fd, /*device_dict=*/true);
    if (rc != PA_OK) return rc;

    // class-list hash table for the count kernel: open addressing of class ids keyed by the hash of the id list
    std::vector<uint32_t> ctab((size_t)fd.num_classes * 2 + 16, 0xFFFFFFFFu);
    for (uint32_t c = 0; c < fd.num_classes; ++c) {
        uint64_t j = list_hash_host(fd.ec.data() + 4ull * fd.class_ref[c] + 1, fd.class_len[c]) % ctab.size();
        while (ctab[j] != 0xFFFFFFFFu)
            if (++j == ctab.size()) j = 0;
        ctab[j] = c;
    }

    pa_index* idx = new (std::nothrow) pa_index();
    if (!idx) return fail(PA_ERR_OOM, "out of memory");
    idx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) idx->num_cus = prop.multiProcessorCount;
    if (idx->num_cus <= 0) idx->num_cus = 256;
    rc = upload(idx->d_blobs, fd.blobs);
    if (rc == PA_OK) rc = upload(idx->d_ledge, fd.ledge);
    if (rc == PA_OK) rc = device_fill_index(fd, idx->d_blobs.get(), idx->d_table, &fd.nbuckets, &fd.dict_pairs);
    if (rc == PA_OK) rc = upload(idx->d_seg_g, fd.seg_g);
    if (rc == PA_OK) rc = upload(idx->d_seg_nid, fd.seg_nid);
    if (rc == PA_OK) rc = upload(idx->d_ec, fd.ec);
    if (rc == PA_OK) rc = upload(idx->d_class_ref, fd.class_ref);
    if (rc == PA_OK) rc = upload(idx->d_class_len, fd.class_len);
    if (rc == PA_OK) rc = upload(idx->d_class_table, ctab);
    if (rc == PA_OK) rc = upload(idx->d_wtable, fd.wtable);
    if (rc != PA_OK) { pa_index_destroy(idx); return rc; }
    idx->class_table_size = ctab.size();
    idx->dv = fd.host_view();
    idx->dv.table = idx->d_table.get();
    idx->dv.blobs = idx->d_blobs.get();
    idx->dv.ledge = idx->d_ledge.get();
    idx->dv.seg_g = idx->d_seg_g.get();
    idx->dv.seg_nid = idx->d_seg_nid.get();
    idx->h_ec = fd.ec;   // host copy of the class table: pa_map_batch resolves by-reference classes from it
    idx->h_class_ref = fd.class_ref;
    idx->h_class_len = fd.class_len;
    idx->dv.ec = idx->d_ec.get();
    idx->dv.class_ref = idx->d_class_ref.get();
    idx->dv.class_len = idx->d_class_len.get();
    idx->dv.wtable = idx->d_wtable.get();
    // a dictionary beyond the Infinity Cache (256 MB) is streamed past the caches (ld_stream): every line of it is used once per probe,
    // and left to itself it evicts the chain blocks, which every read comes back to
    idx->dv.stream_nt = (fd.k <= 32 && dict_table_words(fd.nbuckets, fd.dict_pairs) * 4 > (512ull << 20)) ? 1u : 0u;   // (the two-word dictionary's probe is four loads of one line: slower with the hint)
    pa_index_stats& s = idx->stats;
    s.num_kmers = fd.num_kmers;
    s.table_slots = dict_table_words(fd.nbuckets, fd.dict_pairs) / SLOT_WORDS;
    s.bytes_table = dict_table_words(fd.nbuckets, fd.dict_pairs) * 4;
    s.bytes_graph = fd.blobs.size() + fd.ledge.size() * 4 + fd.seg_g.size() * 12;
    s.bytes_classes = (fd.ec.size() + fd.class_ref.size() + fd.class_len.size() + ctab.size() + fd.wtable.size()) * 4;
    s.bytes_total = s.bytes_table + s.bytes_graph + s.bytes_classes;
    s.num_nodes = fd.num_nodes;
    s.num_classes = fd.num_classes;
    s.k = fd.k;
    s.max_class_len = fd.max_class_len;
    *out = idx;
    return PA_OK;
}

int pa_index_create_multi(const pa_flat_index* flat, const int* devices, int ndev, pa_index** out) {
    if (!flat || !devices || !out || ndev < 1) return fail(PA_ERR_INVALID_ARG, "null argument or ndev < 1");
    for (int i = 0; i < ndev; ++i) out[i] = nullptr;
    for (int i = 0; i < ndev; ++i) {
        for (int j = 0; j < i; ++j)
            if (devices[j] == devices[i]) {
                for (int t = 0; t < i; ++t) { pa_index_destroy(out[t]); out[t] = nullptr; }
                return fail(PA_ERR_INVALID_ARG, "device %d listed twice", devices[i]);
            }
        const int rc = pa_index_create(flat, devices[i], &out[i]);
        if (rc != PA_OK) {
            const std::string why = last_error_ref();
            for (int t = 0; t <= i; ++t) { pa_index_destroy(out[t]); out[t] = nullptr; }
            return fail(rc, "device %d: %s", devices[i], why.c_str());
        }
    }
    return PA_OK;
}

// TEST SURFACE, not part of include/pseudoaligner_amd.h: the dictionary of `flat` as the CPU flattener builds it (device < 0) or as the GPU filler
// builds it on `device`, `builds` times over from the same uploaded blocks. out[cap bytes] receives the first table, *bytes its size, *dict_pairs its
// format (DevIndexView::dict_pairs), *differing the number of later builds whose bytes are not the first one's.
int padbg_dict_table(const pa_flat_index* flat, int device, uint32_t builds, void* out, uint64_t cap, uint64_t* bytes, uint32_t* dict_pairs, uint32_t* differing) {
    if (!flat || !bytes || !dict_pairs || !differing) return fail(PA_ERR_INVALID_ARG, "null argument");
    FlatDevice fd;
    int threads = usable_threads();
    if (threads < 1) threads = 1;
    *differing = 0;
    if (device < 0) {
        const int rc = flatten_for_device(*flat, threads, fd, /*device_dict=*/false);
        if (rc != PA_OK) return rc;
        *bytes = fd.table.size() * 4;
        *dict_pairs = fd.dict_pairs;
        if (out && cap >= *bytes) memcpy(out, fd.table.data(), *bytes);
        return PA_OK;
    }
    int rc = use_device(device);
    if (rc == PA_OK) rc = flatten_for_device(*flat, threads, fd, /*device_dict=*/true);
    DeviceBuffer<uint8_t> d_blobs;
    if (rc == PA_OK) rc = upload(d_blobs, fd.blobs);
    std::vector<uint8_t> again;
    for (uint32_t i = 0; rc == PA_OK && i < builds; ++i) {
        DeviceBuffer<uint32_t> d_table;
        rc = device_fill_index(fd, d_blobs.get(), d_table, &fd.nbuckets, &fd.dict_pairs);
        if (rc != PA_OK) break;
        const uint64_t n = dict_table_words(fd.nbuckets, fd.dict_pairs) * 4;
        if (i == 0) {
            *bytes = n;
            *dict_pairs = fd.dict_pairs;
            if (!out || cap < n) return PA_OK;   // (sizing call)
            if (hipMemcpy(out, d_table.get(), n, hipMemcpyDeviceToHost) != hipSuccess) return fail(PA_ERR_HIP, "hipMemcpy failed");
        } else {
            again.resize(n);
            if (hipMemcpy(again.data(), d_table.get(), n, hipMemcpyDeviceToHost) != hipSuccess) return fail(PA_ERR_HIP, "hipMemcpy failed");
            if (n != *bytes || memcmp(again.data(), out, n) != 0) ++*differing;
        }
    }
    return rc;
}

int pa_index_get_stats(const pa_index* idx, pa_index_stats* stats) {
    if (!idx || !stats) return fail(PA_ERR_INVALID_ARG, "null argument");
    *stats = idx->stats;
    return PA_OK;
}

uint32_t pa_words_per_read(uint32_t max_read_len) { return (max_read_len + 31) / 32 ? (max_read_len + 31) / 32 : 1; }
size_t pa_tiles_words(uint64_t n_reads, uint32_t words_per_read) { return (size_t)((n_reads + 63) / 64) * words_per_read * 64; }

int pa_encode_reads_device(const pa_index* idx, const uint8_t* d_ascii, const uint64_t* d_offsets, uint64_t n_reads,
                           uint32_t words_per_read, uint64_t* d_tiles, uint32_t* d_lens, void* stream) {
    if (!idx || !d_ascii || !d_offsets || !d_tiles || !d_lens || words_per_read == 0) return fail(PA_ERR_INVALID_ARG, "null argument");
    PA_HIP_TRY(hipSetDevice(idx->device));
    const int e = launch_encode(d_ascii, d_offsets, n_reads, words_per_read, d_tiles, d_lens, static_cast<hipStream_t>(stream));
    if (e) return fail(PA_ERR_HIP, "encode launch: %s", hipGetErrorString((hipError_t)e));
    return PA_OK;
}

}  // extern "C"

namespace pa {

// ---- launch geometry ----
static int env_int(const char* name, int dflt) { return knob_int(name, dflt); }   // A/B knobs: -DPA_DEBUG_KNOBS builds only (pa_common.hpp)

// u32 words of a slot's row in the spill / trace scratch: list-mode header + (ref, len, class id, -) quads for >= 2 * max
// read length + 2 node visits; also the stride of the node lists of pa_map_batch_nodes
uint32_t spill_cap_of(uint32_t wpr) { return 256 * wpr + 24; }

// pooled kernel: slots per wave such that `per_cu` workgroups share the 160 KiB of LDS of a CU
static int pool_geometry(pa_index* idx, uint64_t n_reads, uint32_t wpr, uint32_t* grid, size_t* lds, uint32_t* slots) {
    const size_t cu_lds = 160 * 1024 - 4096;   // LDS is allocated in granules: a pool sized to the last byte loses a whole workgroup per CU
    int per_cu = env_int("PA_MAP_BLOCKS_PER_CU", 3);
    uint32_t S = 0;
    for (; per_cu >= 1; --per_cu) {
        const size_t per_wave = cu_lds / (size_t)per_cu / (PA_MAP_BLOCK / 64);
        const size_t per_slot = pool_slot_bytes(wpr);
        if (per_wave < pool_fixed_bytes() + 64 * per_slot + 16) continue;
        S = (uint32_t)((per_wave - pool_fixed_bytes() - 16) / per_slot);
        break;
    }
    if (S < 64) return fail(PA_ERR_UNSUPPORTED, "reads of %u words do not fit the LDS of a compute unit", wpr);
    if (S > pool_max_slots()) S = pool_max_slots();
    const int want = env_int("PA_POOL_SLOTS", 0);
    if (want >= 64 && (uint32_t)want <= S) S = (uint32_t)want;
    *slots = S;
    *lds = pool_lds_bytes(wpr, S);
    int occ = 0;
    if (pool_kernel_occupancy(*lds, &occ) == 0 && occ >= 1 && occ < per_cu) per_cu = occ;
    const uint64_t ntiles = (n_reads + 63) / 64;
    const uint64_t waves_wanted = (ntiles + 7) / 8;                      // >= 8 tiles per wave when the batch allows
    uint64_t blocks = (waves_wanted + PA_MAP_BLOCK / 64 - 1) / (PA_MAP_BLOCK / 64);
    const uint64_t cap = (uint64_t)idx->num_cus * per_cu;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    *grid = (uint32_t)blocks;
    return PA_OK;
}

// the launch context of a stream (created on first use, with the index's device current)
static int ctx_of(pa_index* idx, hipStream_t stream, std::shared_ptr<LaunchCtx>* out) {
    std::lock_guard<std::mutex> g(idx->mu);
    auto it = idx->ctxs.find(stream);
    if (it == idx->ctxs.end()) {
        std::shared_ptr<LaunchCtx> c(new (std::nothrow) LaunchCtx());
        if (!c) return fail(PA_ERR_OOM, "out of memory");
        const int rc = grow(c->ctl, 2);
        if (rc != PA_OK) return rc;
        it = idx->ctxs.emplace(stream, std::move(c)).first;
    }
    *out = it->second;
    return PA_OK;
}

int StreamCtx::open(pa_index* idx, hipStream_t stream) {
    PA_HIP_TRY(hipSetDevice(idx->device));
    const int rc = ctx_of(idx, stream, &cx);
    if (rc != PA_OK) return rc;
    lock = std::unique_lock<std::mutex>(cx->mu);
    return PA_OK;
}

int map_launch_locked(pa_index* idx, LaunchCtx* cx, hipStream_t stream, const MapLaunch& m) {
    const uint64_t n_reads = m.n_reads;
    const uint32_t wpr = m.wpr;
    MapCtl* const ctl = cx->ctl.get();
    if (n_reads >= 0xFFFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "at most 2^32-2 reads per batch");
    if (wpr == 0 || wpr > (PA_MAX_READ_LEN + 31) / 32) return fail(PA_ERR_UNSUPPORTED, "words_per_read %u outside [1,%u]", wpr, (PA_MAX_READ_LEN + 31) / 32);
    uint32_t grid = 0;
    size_t lds = 0;
    uint32_t slots = 64;
    int rc = pool_geometry(idx, n_reads, wpr, &grid, &lds, &slots);
    if (rc != PA_OK) return rc;
    const uint32_t spill_cap = spill_cap_of(wpr);
    {   // long reads: rows of many KB per slot; fewer workgroups keep the scratch at a few GB (throughput of such batches is not the point)
        const size_t per_block = (size_t)(PA_MAP_BLOCK / 64) * slots * spill_cap * 4 * (m.nodes ? 2 : 1);
        const size_t budget = (size_t)6 << 30;
        if ((size_t)grid * per_block > budget) grid = (uint32_t)std::max<size_t>(1, budget / per_block);
    }
    const size_t lanes = (size_t)grid * (PA_MAP_BLOCK / 64) * slots;
    rc = grow(cx->spill, lanes * spill_cap);
    if (rc != PA_OK) return rc;
    if (m.nodes) { rc = grow(cx->trace, lanes * spill_cap); if (rc != PA_OK) return rc; }
    PA_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(MapCtl), stream));
    MapParams p{};
    p.ix = idx->dv;
    p.tiles = m.tiles;
    p.lens = m.lens;
    p.uniform_len = m.uniform_len;
    p.n_reads = n_reads;
    p.wpr = wpr;
    p.allowed = m.allowed;
    p.results = m.results;
    p.arena = m.arena;
    // bit 31 of class_off means "class by reference" (PA_CLASS_REF): offsets handed out by the arena must stay below 2^31
    p.arena_cap = m.arena_cap > PA_MAX_ARENA_ENTRIES ? PA_MAX_ARENA_ENTRIES : m.arena_cap;
    p.colour_out = m.colour;
    p.arena_top = &ctl->arena_top;
    p.status = &ctl->status;
    p.tile_ctr = &ctl->tile_ctr;
    p.spill = cx->spill.get();
    p.spill_cap = spill_cap;
    const uint64_t counts_len = (uint64_t)idx->stats.num_classes + 3;
    // reads whose class has to be looked up by content are resolved after the launch (resolve.hip): 8 words per read in the worst case
    const uint64_t defer_cap = defer_capacity(n_reads, grid * (PA_MAP_BLOCK / 64));
    if ((rc = grow(cx->defer, defer_cap * 8))) return rc;
    p.defer = cx->defer.get();
    p.defer_top = &ctl->defer_top;
    p.defer_cap = defer_cap;
    p.keys_cap = 0;
    uint64_t keys_cap = 0;
    if (m.counts) {   // the waves' key streams (4.3 bytes per read), one key per deferred read behind them, and the keys partitioned by bin (2 bytes per key)
        keys_cap = key_stream_capacity(n_reads, grid * (PA_MAP_BLOCK / 64));
        size_t sorted_bytes = 0, ctl_bytes = 0;
        count_keys_scratch(counts_len, n_reads, keys_cap, defer_cap, &sorted_bytes, &ctl_bytes);
        if ((rc = grow(cx->keys, keys_cap + defer_cap)) || (rc = grow(cx->keys_sorted, (sorted_bytes + 3) / 4)) || (rc = grow(cx->keys_ctl, (ctl_bytes + 3) / 4))) return rc;
        p.keys = cx->keys.get();
        p.keys_top = &ctl->keys_top;
        p.keys_cap = keys_cap;
        p.counts = reinterpret_cast<unsigned long long*>(m.counts);
    }
    p.class_table = idx->d_class_table.get();
    p.class_table_size = idx->class_table_size;
    p.pool_slots = slots;
    p.dbg = env_int("PA_MAP_STATS", 0) ? ctl->stats : nullptr;
    p.ablate = (uint32_t)env_int("PA_MAP_ABLATE", 0);
    pa_overflow* ovf = nullptr;
    { std::lock_guard<std::mutex> g(idx->mu); ovf = idx->ovf; }
    if (m.counts && ovf) {   // novel results of this launch are listed (per stream) for the overflow table
        const uint64_t want = n_reads + 64;   // every read can end in a novel class: the list never overflows
        rc = grow(cx->novel, want * 2);
        if (rc != PA_OK) return rc;
        p.novel_list = cx->novel.get();
        p.novel_ctr = &ctl->novel_ctr;
        p.novel_cap = want;
        overflow_launch_params(ovf, p);
    }
    p.trace = m.nodes ? cx->trace.get() : nullptr;
    p.nodes_out = m.nodes;
    p.nodes_len = m.nodes_len;
    cx->last_grid = grid;
    cx->last_arena_cap = p.arena_cap;
    cx->timed = false;
    if (n_reads == 0) return PA_OK;
    bool timing = false;
    { std::lock_guard<std::mutex> g(idx->mu); timing = idx->timing; }
    if (timing) {
        if (!cx->ev0) { PA_HIP_TRY(hipEventCreate(&cx->ev0)); PA_HIP_TRY(hipEventCreate(&cx->ev1)); PA_HIP_TRY(hipEventCreate(&cx->ev2)); PA_HIP_TRY(hipEventCreate(&cx->ev3)); }
        PA_HIP_TRY(hipEventRecord(cx->ev0, stream));
    }
    const int e = launch_map_pool(p, grid, lds, stream);
    if (e) return fail(PA_ERR_HIP, "map launch (grid %u, lds %zu): %s", grid, lds, hipGetErrorString((hipError_t)e));
    if (timing) { PA_HIP_TRY(hipEventRecord(cx->ev1, stream)); cx->timed = true; }
    // resolve and the partition of the map kernel's keys need only the map kernel: with a partitioned table they run side by side
    // (resolve on cx->side); the partition of the deferred reads' keys, the count kernel and the overflow table wait for both
    const bool overlap = m.counts && count_keys_partitioned(counts_len, n_reads);
    hipStream_t rs = stream;
    if (overlap) {
        if (!cx->side) {
            PA_HIP_TRY(hipStreamCreateWithFlags(&cx->side, hipStreamNonBlocking));
            PA_HIP_TRY(hipEventCreateWithFlags(&cx->fork, hipEventDisableTiming));
            PA_HIP_TRY(hipEventCreateWithFlags(&cx->join, hipEventDisableTiming));
        }
        PA_HIP_TRY(hipEventRecord(cx->fork, stream));
        PA_HIP_TRY(hipStreamWaitEvent(cx->side, cx->fork, 0));
        rs = cx->side;
    }
    {
        const int e1 = launch_resolve(p, defer_cap, keys_cap, idx->num_cus, rs);
        if (e1) return fail(PA_ERR_HIP, "resolve launch: %s", hipGetErrorString((hipError_t)e1));
    }
    if (timing) PA_HIP_TRY(hipEventRecord(cx->ev2, rs));
    if (overlap) {
        PA_HIP_TRY(hipEventRecord(cx->join, rs));
        const int e2 = launch_count_keys(p.keys, p.keys_top, keys_cap, p.defer_top, defer_cap, cx->keys_sorted.get(), cx->keys_ctl.get(), p.counts, counts_len,
                                         idx->num_cus, stream, n_reads, 0);
        if (e2) return fail(PA_ERR_HIP, "count launch: %s", hipGetErrorString((hipError_t)e2));
        PA_HIP_TRY(hipStreamWaitEvent(stream, cx->join, 0));
    }
    if (m.counts) {
        const int e2 = launch_count_keys(p.keys, p.keys_top, keys_cap, p.defer_top, defer_cap, cx->keys_sorted.get(), cx->keys_ctl.get(), p.counts, counts_len,
                                         idx->num_cus, stream, n_reads, 1);
        if (e2) return fail(PA_ERR_HIP, "count launch: %s", hipGetErrorString((hipError_t)e2));
        if (ovf) {
            rc = overflow_after_map(ovf, p.novel_list, p.novel_ctr, p.novel_cap, m.arena, stream);
            if (rc != PA_OK) return rc;
        }
    }
    if (timing) PA_HIP_TRY(hipEventRecord(cx->ev3, stream));
    return PA_OK;
}

int map_finish_locked(LaunchCtx* cx, hipStream_t stream, uint64_t* arena_used, uint64_t* arena_needed) {
    // (the head of the control block comes back ON the launch's stream: a plain hipMemcpy runs on the null stream and waits for every other stream
    // of the process — a caller that copies its next batch in on another stream meanwhile would find this call waiting for that copy)
    MapCtl ctl{};
    PA_HIP_TRY(hipMemcpyAsync(&ctl, cx->ctl.get(), offsetof(MapCtl, stats), hipMemcpyDeviceToHost, stream));
    PA_HIP_TRY(hipStreamSynchronize(stream));
    if (env_int("PA_MAP_STATS", 0)) {
        PA_HIP_TRY(hipMemcpy(&ctl, cx->ctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
        static const char* names[] = {"refill", "seek", "fwd", "left", "pick+pop", "store+push", "fin_light", "fin_scan", "fin_coop", "fin_bits", "fin_mask", "fwd+seek", "fwd:issue", "fwd:wait", "fwd:wait+compute"};
        static_assert(sizeof names / sizeof names[0] == ST_NSTAT, "one name per statistics entry");
        const unsigned long long* d = ctl.stats;
        fprintf(stderr, "[pa map stats] grid=%u", cx->last_grid);
        for (uint32_t i = 0; i < ST_NSTAT; ++i)
            if (d[i])
                fprintf(stderr, " %s: %llu iters x %.1f lanes, %.0f ticks/iter;", names[i], d[i], (double)d[ST_NSTAT + i] / (double)d[i],
                        (double)d[2 * ST_NSTAT + i] / (double)d[i]);
        fprintf(stderr, " key stream %llu entries, deferred stream %llu entries\n", ctl.keys_top, ctl.defer_top);
    }
    // the counter includes every wave's partly used chunk and may run past the caller's arena without any allocation having
    // crossed its end: what may be copied back is min(top, capacity); `needed` is the capacity that would have sufficed
    const unsigned long long top = ctl.arena_top;
    if (arena_used) *arena_used = top < cx->last_arena_cap ? top : cx->last_arena_cap;
    if (arena_needed) *arena_needed = top;
    if (ctl.status & PA_STATUS_SPILL_OVERFLOW) return fail(PA_ERR_INTERNAL, "a per-launch stream (class rows, count keys or deferred reads) overflowed its buffer (should be impossible)");
    if (ctl.status & PA_STATUS_ARENA_FULL) return fail(PA_ERR_ARENA_FULL, "class arena too small: %llu entries needed", top);
    return PA_OK;
}

}  // namespace pa

// the one path of the device entry points: device, context of the stream, lock, launch
static int map_launch(pa_index* idx, void* stream, const MapLaunch& m) {
    StreamCtx s;
    const int rc = s.open(idx, static_cast<hipStream_t>(stream));
    if (rc != PA_OK) return rc;
    return map_launch_locked(idx, s.cx.get(), static_cast<hipStream_t>(stream), m);
}

// the context of `stream`, locked, once a timed launch has run on it
static int timed_ctx(pa_index* idx, void* stream, const void* ms, StreamCtx* s) {
    if (!idx || !ms) return fail(PA_ERR_INVALID_ARG, "null argument");
    const int rc = s->open(idx, static_cast<hipStream_t>(stream));
    if (rc != PA_OK) return rc;
    if (!s->cx->timed) return fail(PA_ERR_INVALID_ARG, "no timed launch on this stream (pa_index_set_timing before the launch)");
    return PA_OK;
}

extern "C" {

// The launch context of `stream` (control block, list-mode rows, key / deferred-read streams, novel list: 2 GB + 45 bytes per read at 150 bp on a 256-CU
// part) is freed; the next launch on that stream creates a fresh one. Callers that create and destroy streams call this
// before hipStreamDestroy — a context left behind would stay until pa_index_destroy and could be matched to a later stream
// whose handle value the runtime reuses.
int pa_index_release_stream(pa_index* idx, void* stream) {
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    std::shared_ptr<LaunchCtx> cx;
    {
        std::lock_guard<std::mutex> g(idx->mu);
        auto it = idx->ctxs.find(static_cast<hipStream_t>(stream));
        if (it == idx->ctxs.end()) return PA_OK;
        cx = std::move(it->second);
        idx->ctxs.erase(it);
    }
    std::lock_guard<std::mutex> g(cx->mu);   // (a launch in progress on another thread finishes first; one that only holds the pointer yet finds empty buffers and re-creates them)
    hipError_t e = hipSetDevice(idx->device);
    if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    cx->release();                           // also on the error path: the context is no longer reachable from the index
    if (e != hipSuccess) return fail(PA_ERR_HIP, "pa_index_release_stream: %s", hipGetErrorString(e));
    return PA_OK;
}

int pa_map_batch_device(pa_index* idx, const uint64_t* d_tiles, const uint32_t* d_lens, uint64_t n_reads, uint32_t words_per_read,
                        uint32_t allowed_mismatches, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                        uint32_t* d_colour, void* stream) {
    if (!idx || (n_reads && (!d_tiles || !d_lens || !d_results || !d_arena))) return fail(PA_ERR_INVALID_ARG, "null argument");
    MapLaunch m;
    m.tiles = d_tiles; m.lens = d_lens; m.n_reads = n_reads; m.wpr = words_per_read; m.allowed = allowed_mismatches;
    m.results = d_results; m.arena = d_arena; m.arena_cap = arena_cap; m.colour = d_colour;
    return map_launch(idx, stream, m);
}

int pa_map_count_batch_device(pa_index* idx, const uint64_t* d_tiles, const uint32_t* d_lens, uint64_t n_reads, uint32_t words_per_read,
                              uint32_t allowed_mismatches, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap,
                              uint64_t* d_counts, void* stream) {
    if (!idx || !d_counts || (n_reads && (!d_tiles || !d_lens || !d_results || !d_arena))) return fail(PA_ERR_INVALID_ARG, "null argument");
    MapLaunch m;
    m.tiles = d_tiles; m.lens = d_lens; m.n_reads = n_reads; m.wpr = words_per_read; m.allowed = allowed_mismatches;
    m.results = d_results; m.arena = d_arena; m.arena_cap = arena_cap; m.counts = d_counts;
    return map_launch(idx, stream, m);
}

int pa_map_count_batch_uniform_device(pa_index* idx, const uint64_t* d_tiles, uint32_t read_len, uint64_t n_reads, uint32_t words_per_read,
                                      uint32_t allowed_mismatches, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts,
                                      void* stream) {
    if (!idx || !d_counts || (n_reads && (!d_tiles || !d_results || !d_arena))) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (read_len == 0 || read_len > PA_MAX_READ_LEN || read_len > 32ull * words_per_read)
        return fail(PA_ERR_INVALID_ARG, "read_len %u does not fit %u words per read (or exceeds %u bases)", read_len, words_per_read, PA_MAX_READ_LEN);
    MapLaunch m;
    m.tiles = d_tiles; m.uniform_len = read_len; m.n_reads = n_reads; m.wpr = words_per_read; m.allowed = allowed_mismatches;
    m.results = d_results; m.arena = d_arena; m.arena_cap = arena_cap; m.counts = d_counts;
    return map_launch(idx, stream, m);
}

int pa_map_finish(pa_index* idx, void* stream, uint64_t* arena_used, uint64_t* arena_needed) {
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    StreamCtx s;
    const int rc = s.open(idx, static_cast<hipStream_t>(stream));
    if (rc != PA_OK) return rc;
    return map_finish_locked(s.cx.get(), static_cast<hipStream_t>(stream), arena_used, arena_needed);
}

int pa_index_set_timing(pa_index* idx, int on) {
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> g(idx->mu);
    idx->timing = on != 0;
    return PA_OK;
}

int pa_map_kernel_ms(pa_index* idx, void* stream, float* ms) {
    StreamCtx s;
    const int rc = timed_ctx(idx, stream, ms, &s);
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipEventSynchronize(s.cx->ev1));
    PA_HIP_TRY(hipEventElapsedTime(ms, s.cx->ev0, s.cx->ev1));
    return PA_OK;
}

int pa_map_stage_ms(pa_index* idx, void* stream, float ms[3]) {
    StreamCtx s;
    const int rc = timed_ctx(idx, stream, ms, &s);
    if (rc != PA_OK) return rc;
    PA_HIP_TRY(hipEventSynchronize(s.cx->ev3));
    PA_HIP_TRY(hipEventElapsedTime(&ms[0], s.cx->ev0, s.cx->ev1));
    PA_HIP_TRY(hipEventElapsedTime(&ms[1], s.cx->ev1, s.cx->ev2));
    PA_HIP_TRY(hipEventElapsedTime(&ms[2], s.cx->ev2, s.cx->ev3));
    return PA_OK;
}

uint64_t pa_map_arena_hint(const pa_index* idx, uint64_t n_reads) {
    // enough for ~8 ids per read plus one partially used chunk per wave; pa_map_finish reports the exact need
    const uint64_t waves = idx ? (uint64_t)idx->num_cus * 8 * (PA_MAP_BLOCK / 64) : 8192;
    return n_reads * 8 + waves * PA_ARENA_CHUNK + 4096;
}

int pa_counts_by_barcode_device(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena, const uint32_t* d_barcode, uint64_t n_reads,
                                uint32_t barcode_bits, uint64_t* d_keys, uint32_t* d_vals, uint64_t* n_entries, void* stream) {
    if (!idx || !n_entries || (n_reads && (!d_results || !d_arena || !d_barcode || !d_keys || !d_vals))) return fail(PA_ERR_INVALID_ARG, "null argument");
    PA_HIP_TRY(hipSetDevice(idx->device));
    return barcode_counts(idx->dv, idx->d_class_table.get(), idx->class_table_size, d_results, d_arena, d_barcode, n_reads,
                          barcode_bits, d_keys, d_vals, n_entries, static_cast<hipStream_t>(stream));
}

int pa_index_set_overflow(pa_index* idx, pa_overflow* ovf) {
    if (!idx) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (ovf && overflow_device(ovf) != idx->device) return fail(PA_ERR_INVALID_ARG, "overflow table lives on device %d, the index on device %d", overflow_device(ovf), idx->device);
    std::lock_guard<std::mutex> g(idx->mu);
    idx->ovf = ovf;
    return PA_OK;
}

// ---- counts ----
uint64_t pa_counts_len(const pa_index* idx) { return idx ? (uint64_t)idx->stats.num_classes + 3 : 0; }

int pa_counts_accumulate_device(pa_index* idx, const pa_read_result* d_results, const uint32_t* d_arena, const uint32_t* d_colour,
                                uint64_t n_reads, uint64_t* d_counts, void* stream) {
    if (!idx || !d_results || !d_arena || !d_counts) return fail(PA_ERR_INVALID_ARG, "null argument");
    PA_HIP_TRY(hipSetDevice(idx->device));
    const int e = launch_count(d_results, d_arena, d_colour, n_reads, idx->dv, idx->d_class_table.get(),
                               idx->class_table_size, reinterpret_cast<unsigned long long*>(d_counts), static_cast<hipStream_t>(stream));
    if (e) return fail(PA_ERR_HIP, "count launch: %s", hipGetErrorString((hipError_t)e));
    return PA_OK;
}

}  // extern "C"
