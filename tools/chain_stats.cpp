// Tuning aid (CPU only): what does the chain-block layout (device_layout.hpp) do to a workload? Builds the index of a workload,
// flattens it, and runs the product's lane state machine on the host (as tests/emu does) over simulated reads: chains per node,
// blocks, and per read the dictionary probes, forward / left steps and DISTINCT 128-byte chain blocks fetched — the unit the
// memory system moves and the mapping kernel is bound by.
//
//   g++ -O2 -std=c++17 -pthread tools/chain_stats.cpp rust-pseudoaligner_amd/csrc/{host_index,dbg_build,device_flatten,synth}.cpp -lz -o /tmp/chain_stats
//   /tmp/chain_stats [--kernel] [--no-cache] <k> <read_len> <ppm> <n_reads> [fasta]
//
// The forward step has two texts (lane_steps.hpp): the GENERAL one (any number of nodes per step; traced batches, careful and list mode)
// and the straight-line one the kernel's common lanes take (two nodes per step). The figures above are those of the general step, which
// also yields the node trace the hop statistics need. --kernel steps the reads a second time as the kernel does (fwd_step<false>) and
// prints both side by side: forward steps, distinct blocks, what the later steps of a walk do, and the steps that have to look for
// their node's slot. --no-cache builds the index instead of reusing /tmp/chain_stats_*.idx (which is keyed by k only, not by the FASTA).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../rust-pseudoaligner_amd/csrc/device_flatten.hpp"
#include "../rust-pseudoaligner_amd/csrc/dict_slots.hpp"
#include "../rust-pseudoaligner_amd/csrc/lane_steps.hpp"
#include "../rust-pseudoaligner_amd/csrc/pa_common.hpp"

using namespace pa;

struct PassStats {
    uint64_t n_unknown = 0, n_seek = 0, n_fwd = 0, n_left = 0, n_blocks = 0, n_nodes = 0, n_lists = 0, hop_edges = 0, hop_unique = 0, hop_unique_rem = 0;
    // forward steps after which the lane goes on FORWARD, by where its next step reads: a chain entered over an edge, another chain
    // through a link, the block it holds, another block of its chain (re-based) — and of the latter those whose rest of the read
    // would have fitted the block the lane held
    uint64_t next_edge = 0, next_link = 0, next_same = 0, next_rebased = 0, rebased_fits = 0;
    std::map<uint32_t, uint64_t> rem_hist, fwd_hist;
};

// every read of the batch stepped to the end of its walk; KERNEL: the forward step as the kernel's common lanes take it
template <bool KERNEL>
static void run_pass(const DevIndexView& ix, const pa_flat_index& f, const std::vector<uint64_t>& tiles, const std::vector<uint32_t>& lens, uint32_t wpr,
                     uint32_t read_len, PassStats& st) {
    const uint64_t n = lens.size();
    std::vector<uint64_t> rd(wpr + 2);
    alignas(16) uint32_t refs[4], lens4[4], cids4[4], win4[4];
    uint32_t wcand[2];
    std::vector<uint32_t> spill(8 * read_len + 64), trace(8 * read_len + 64), pend(8 * read_len + 64);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t t = i >> 6, r = i & 63;
        for (uint32_t w = 0; w < wpr; ++w) rd[w] = tiles[(t * wpr + w) * 64 + r];
        rd[wpr] = rd[wpr + 1] = 0;
        Lane s;
        lane_start(s, (uint32_t)i, lens[i], ix.k);
        const ReadRef rr{rd.data(), 1, wpr};
        const ColRef cr{win4, wcand, refs, lens4, cids4, spill.data(), (uint32_t)spill.size(), pend.data(), trace.data()};
        std::vector<uint32_t> blocks;
        uint32_t nf = 0;
        for (;;) {
            while (l_st(s) == ST_SEEK || l_st(s) == ST_FWD || l_st(s) == ST_LEFT) {
                if (l_st(s) == ST_SEEK) { seek_step(s, ix, rr); ++st.n_seek; }
                else if (l_st(s) == ST_FWD) {
                    blocks.push_back(s.h);
                    if (!(s.of & OF_CUR_KNOWN)) ++st.n_unknown;
                    const uint32_t h0 = s.h;
                    fwd_step<!KERNEL>(s, ix, rr, cr, 2);
                    ++st.n_fwd; ++nf;
                    if (l_st(s) == ST_FWD) {
                        if (l_flags(s) & F_FRESH) ++st.next_edge;
                        else if (s.h == h0) ++st.next_same;
                        else if (s.of & OF_CUR_KNOWN) ++st.next_link;
                        else {
                            ++st.next_rebased;
                            const uint32_t x_held = l_off(s) + ((s.h - h0) << CH_STRIDE_LOG2);   // the same base as a position of the block the lane held
                            if (x_held + (l_L(s) - l_kp(s)) <= CH_WINDOW) ++st.rebased_fits;
                        }
                    }
                    if (!KERNEL && l_st(s) == ST_FWD && (l_flags(s) & F_FRESH) && l_ntrace(s)) {   // left its chain over an edge
                        ++st.hop_edges;
                        const uint32_t from = trace[l_ntrace(s) - 1], re = f.node_exts[from] & 15u;
                        if (!(re & (re - 1))) { ++st.hop_unique; st.hop_unique_rem += l_L(s) - (l_kp(s) + ix.k); st.rem_hist[(l_L(s) - (l_kp(s) + ix.k)) / 16]++; }
                    }
                }
                else { blocks.push_back(s.ph); left_step<!KERNEL>(s, ix, rr, cr, 2); ++st.n_left; }
            }
            if (l_st(s) != ST_ISECT || (l_flags(s) & F_LISTS)) break;
            if (window_todo(s) == 2) { restart_lists(s, ix.k); ++st.n_lists; continue; }
            break;
        }
        st.fwd_hist[nf]++;
        st.n_nodes += l_ntrace(s);
        std::sort(blocks.begin(), blocks.end());
        st.n_blocks += std::unique(blocks.begin(), blocks.end()) - blocks.begin();
    }
}

int main(int argc, char** argv) {
    bool kernel = false, no_cache = false;
    std::vector<char*> pos;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--kernel")) kernel = true;
        else if (!strcmp(argv[i], "--no-cache")) no_cache = true;
        else pos.push_back(argv[i]);
    }
    const uint32_t k = pos.size() > 0 ? atoi(pos[0]) : 24, read_len = pos.size() > 1 ? atoi(pos[1]) : 150, ppm = pos.size() > 2 ? atoi(pos[2]) : 0;
    const uint64_t n = pos.size() > 3 ? atoll(pos[3]) : 100000;
    const char* fasta = pos.size() > 4 ? pos[4] : nullptr;
    pa_txome* tx = nullptr;
    if (fasta) { if (pa_txome_from_fasta(fasta, &tx)) { fprintf(stderr, "%s\n", pa_last_error()); return 1; } }
    else if (pa_txome_synthesize(58000, 203000, 7, &tx)) { fprintf(stderr, "%s\n", pa_last_error()); return 1; }
    const uint64_t *packed, *tx_start;
    uint32_t num_tx;
    pa_txome_view(tx, &packed, &tx_start, &num_tx);
    char cache[256];
    snprintf(cache, sizeof cache, "/tmp/chain_stats_%s_k%u.idx", fasta ? "fasta" : "synth", k);
    pa_host_index* h = nullptr;
    if (no_cache || pa_host_index_load(cache, &h) != PA_OK) {
        if (pa_host_index_build_packed(packed, tx_start, num_tx, k, 8, &h)) { fprintf(stderr, "%s\n", pa_last_error()); return 1; }
        if (!no_cache) pa_host_index_save(h, cache);
    }
    pa_flat_index f;
    pa_host_index_view(h, &f);
    FlatDevice fd;
    if (flatten_for_device(f, 8, fd, false)) { fprintf(stderr, "%s\n", pa_last_error()); return 1; }
    const DevIndexView ix = fd.host_view();
    uint64_t mergeable = 0;
    {
        // nodes whose only right extension leads to a node whose only left extension leads back (what a chain may merge)
        for (uint32_t i = 0; i < f.num_nodes; ++i) {
            const uint32_t re = f.node_exts[i] & 15u;
            if (re && !(re & (re - 1))) ++mergeable;   // upper bound (the successor's left side is not checked here)
        }
    }
    printf("index: %u nodes (%llu with one right extension), %u chains, %zu blocks (%.1f MB), %u classes\n", f.num_nodes, (unsigned long long)mergeable,
           fd.num_chains, fd.blobs.size() / CH_BLOCK, fd.blobs.size() / 1e6, f.num_classes);
    if (fd.dict_pairs) {   // the pair dictionary: where its keys lie (device_layout.hpp: a tag's displacement field)
        const uint64_t* e = reinterpret_cast<const uint64_t*>(fd.table.data());
        const uint64_t n = 2ull << fd.dict_pairs;
        uint64_t keys = 0, off_home = 0;
        uint32_t furthest = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (e[i] == PAIR_EMPTY) continue;
            const uint32_t d = pair_entry_tag(e[i]) >> (PAIR_KEY_BITS - fd.dict_pairs);
            ++keys;
            off_home += d != 0;
            furthest = std::max(furthest, d);
        }
        printf("pair dictionary: 2^%u pairs (%.2f GB), %.3f keys per pair, %llu of %llu keys off their home pair (%.2f %%), the furthest %u pairs on\n", fd.dict_pairs,
               16.0 * (double)(1ull << fd.dict_pairs) / 1e9, (double)keys / (double)(1ull << fd.dict_pairs), (unsigned long long)off_home, (unsigned long long)keys,
               100.0 * (double)off_home / (double)keys, furthest);
    }
    // slot use per block
    {
        uint64_t hist[5] = {0, 0, 0, 0, 0};
        for (size_t b = 0; b + CH_BLOCK <= fd.blobs.size(); b += CH_BLOCK) {
            const uint32_t* sl = reinterpret_cast<const uint32_t*>(fd.blobs.data() + b);
            const uint32_t rm = sl[0] >> SEG_RECMASK_SHIFT;
            uint32_t used = 0;
            for (uint32_t t = 0; t < 4; ++t)
                if ((rm >> t) & 1u) { const uint32_t w0 = sl[4 * t]; used += 1 + ((w0 & SEG_WIDE) ? 1 : 0) + ((w0 & SEG_EDGES) ? 1 : 0); }
            hist[std::min(used, 4u)]++;
        }
        printf("slots used per block: 1:%llu 2:%llu 3:%llu 4:%llu\n", (unsigned long long)hist[1], (unsigned long long)hist[2], (unsigned long long)hist[3], (unsigned long long)hist[4]);
    }
    const uint32_t wpr = (read_len + 31) / 32;
    std::vector<uint64_t> tiles(((n + 63) / 64) * wpr * 64);
    std::vector<uint32_t> lens(n);
    pa_simulate_reads_host(tx, read_len, k == 31 ? 4 : 2, ppm, 0, n, wpr, tiles.data(), lens.data());
    PassStats g;
    run_pass<false>(ix, f, tiles, lens, wpr, read_len, g);
    printf("per read: %.3f probes, %.3f forward steps, %.3f left steps, %.3f distinct chain blocks, %.3f nodes pushed, %.4f list-mode restarts\n", (double)g.n_seek / n,
           (double)g.n_fwd / n, (double)g.n_left / n, (double)g.n_blocks / n, (double)g.n_nodes / n, (double)g.n_lists / n);
    printf("per read: %.3f hops over an edge, %.3f of them from a node with ONE right extension (mean read bases left then: %.1f)\n", (double)g.hop_edges / n,
           (double)g.hop_unique / n, g.hop_unique ? (double)g.hop_unique_rem / g.hop_unique : 0.0);
    printf("forward steps that had to look for their node's slot: %.4f per read\n", (double)g.n_unknown / n);
    printf("forward steps per read:");
    for (auto& kv : g.fwd_hist) printf(" %u:%.3f", kv.first, (double)kv.second / n);
    printf("\n");
    if (kernel) {
        PassStats q;
        run_pass<true>(ix, f, tiles, lens, wpr, read_len, q);
        const double d = (double)n;
        printf("\nper read                                                      general step   as the kernel steps\n");
#define ROW(label, field) printf("%-60s %13.4f %21.4f\n", label, (double)g.field / d, (double)q.field / d);
        ROW("forward steps", n_fwd)
        ROW("distinct 128-byte chain blocks fetched", n_blocks)
        ROW("later steps that hop over an edge", next_edge)
        ROW("later steps that follow a link", next_link)
        ROW("later steps in the same block", next_same)
        ROW("later steps RE-BASED to another block of the same chain", next_rebased)
        ROW("... of which the rest of the read fits the block held", rebased_fits)
        ROW("forward steps that have to LOOK FOR their node's slot", n_unknown)
#undef ROW
        // one line for scripts and tests: exact counts
        printf("kernel_step_counts reads=%llu fwd=%llu blocks=%llu unknown=%llu rebased=%llu rebased_fits=%llu general_fwd=%llu general_blocks=%llu general_unknown=%llu\n",
               (unsigned long long)n, (unsigned long long)q.n_fwd, (unsigned long long)q.n_blocks, (unsigned long long)q.n_unknown, (unsigned long long)q.next_rebased,
               (unsigned long long)q.rebased_fits, (unsigned long long)g.n_fwd, (unsigned long long)g.n_blocks, (unsigned long long)g.n_unknown);
    }
    pa_host_index_destroy(h);
    pa_txome_destroy(tx);
    return 0;
}
