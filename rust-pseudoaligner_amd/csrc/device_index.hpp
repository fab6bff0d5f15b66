// The index handle, the per-stream launch context and the internal launch / finish calls of device_index.hip, for the units that sit on them
// (map_batch.hip). Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "hip_buffer.hpp"
#include "kernels.hpp"
#include "pa_common.hpp"

namespace pa {

// per-launch scratch of one stream
struct LaunchCtx {
    std::mutex mu;
    DeviceBuffer<MapCtl> ctl;
    DeviceBuffer<uint32_t> spill, trace, novel;
    DeviceBuffer<uint32_t> keys, keys_sorted, keys_ctl;   // class-count launches: the waves' key streams (+ one key per deferred read), the keys partitioned by bin inside tiles, where the runs lie (count_sort.hip)
    DeviceBuffer<uint32_t> defer;                         // reads whose class is looked up by content after the launch (resolve.hip): 8 words each, sized for every read
    uint32_t last_grid = 0;
    uint64_t last_arena_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;   // before the map kernel / after it / after the resolve kernel (on `side`) / after the count kernels of the last launch (pa_index_set_timing)
    bool timed = false;
    // class-count launches with a partitioned table: pa_resolve_kernel runs on `side` while the caller's stream partitions the map kernel's
    // keys (fork: the map kernel is done; join: resolve is done). Owned here: it lives and dies with the context of the caller's stream.
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    void release();
};

// Opaque objects a driver parks on the index between calls, at most `cap` of them (allocating their buffers costs more than a batch): take() hands
// one to the caller alone, put() stores it back or, when the list is full, frees it with `free_fn`. Guarded by the index's `mu`.
struct Parked {
    size_t cap;
    std::vector<std::pair<void*, void (*)(void*)>> held;
    void* take(std::mutex& mu);
    void put(std::mutex& mu, void* obj, void (*free_fn)(void*));
};

// one map launch: what the three device entry points and the host-buffer path differ in
struct MapLaunch {
    const uint64_t* tiles = nullptr;
    const uint32_t* lens = nullptr;   // [n_reads], or nullptr: every read has uniform_len bases
    uint32_t uniform_len = 0;
    uint64_t n_reads = 0;
    uint32_t wpr = 0, allowed = 0;
    pa_read_result* results = nullptr;
    uint32_t* arena = nullptr;
    uint64_t arena_cap = 0;
    uint32_t* colour = nullptr;
    uint64_t* counts = nullptr;       // class-count launches: the caller's table
    uint32_t* nodes = nullptr;        // trace launches: per-read node lists (stride spill_cap_of(wpr)) and their lengths
    uint32_t* nodes_len = nullptr;
};

// The launch context of `stream` (created on first use) with its lock held and the index's device current — made current BEFORE the lookup, which
// may allocate the context's control block.
struct StreamCtx {
    std::shared_ptr<LaunchCtx> cx;
    std::unique_lock<std::mutex> lock;
    int open(pa_index* idx, hipStream_t stream);
};

uint32_t spill_cap_of(uint32_t wpr);
// under the context's lock (StreamCtx): the map kernel and what follows it on `stream`; the launch's control block read back on `stream`
int map_launch_locked(pa_index* idx, LaunchCtx* cx, hipStream_t stream, const MapLaunch& m);
int map_finish_locked(LaunchCtx* cx, hipStream_t stream, uint64_t* arena_used, uint64_t* arena_needed);

}  // namespace pa

struct pa_index {
    int device = 0;
    int num_cus = 0;
    pa::DevIndexView dv{};
    pa::DeviceBuffer<uint32_t> d_table, d_ledge, d_seg_nid, d_ec, d_class_ref, d_class_len, d_class_table, d_wtable;
    pa::DeviceBuffer<uint8_t> d_blobs;
    pa::DeviceBuffer<uint64_t> d_seg_g;
    uint64_t class_table_size = 0;
    pa_index_stats stats{};
    // per-launch scratch: one context per stream the caller launches on, so that launches on different streams (from one or
    // several host threads) run concurrently; launches on ONE stream share a context and are ordered by the stream
    std::mutex mu;                // guards `ctxs`, `ovf`, `timing` and the parked objects
    std::map<hipStream_t, std::shared_ptr<pa::LaunchCtx>> ctxs;   // shared: a launch that looked its context up keeps it alive across pa_index_release_stream
    pa_overflow* ovf = nullptr;   // attached overflow table of novel classes (collective.hip), not owned
    bool timing = false;          // pa_index_set_timing: HIP events around the map kernel of every launch
    std::mutex hmu;               // the host-buffer convenience path (b_* below, map_batch.hip) is one batch at a time
    pa::DeviceBuffer<uint8_t> b_ascii;
    pa::DeviceBuffer<uint64_t> b_offsets, b_tiles;
    pa::DeviceBuffer<uint32_t> b_lens, b_arena, b_nodes, b_nodes_len;
    pa::DeviceBuffer<pa_read_result> b_results;
    std::vector<uint32_t> h_class_ids;
    std::vector<uint32_t> h_ec, h_class_ref, h_class_len;
    // every index class rendered once as the reference prints it between the brackets ("1, 5, 9"): text of class c =
    // h_class_text[h_class_text_off[c] .. h_class_text_off[c + 1]). Built on first use by the ingest pipelines (ingest.hpp): a read
    // whose class comes back by reference then costs one copy instead of a table walk and a decimal conversion per id.
    std::once_flag class_text_once;
    std::vector<uint64_t> h_class_text_off;
    std::vector<char> h_class_text;
    std::vector<uint32_t> h_arena;
    pa::DeviceBuffer<uint64_t> d_class_text_off;   // device copy of the rendered classes (uploaded on first use, under `mu`)
    pa::DeviceBuffer<uint8_t> d_class_text;
    // parked between calls: the buffer sets of up to four lanes of fastq_reads.cpp / record_stream.cpp (pa_process_reads_multi with the handle listed
    // several times, concurrent callers), and of pa_map_tiles_host (host_batch.cpp) the streams + staging buffers of the chunks in flight
    pa::Parked ingest_caches{4, {}}, host_pipes{2, {}};
};
