// Unstranded libraries behind the map launch (include/pseudoaligner_amd.h, "unstranded libraries"). An item (a read or a pair)
// arrives with two candidate results, S (as given) and R (the other strand), each ordinary pa_read_result records plus arena ids; the stage of
// pair_stage.hpp merges them per item by the rule of the header into ordinary records plus ids in its own arena. StrandRule is that rule:
//
//   classify  the record of every item that needs no id traffic is final (neither candidate mapped; a winner whose class is empty or given by
//             reference; a tie of the same reference twice; a tie of two empties); the others get the WORK KEY: the length of the winner's
//             list, or na + nb for the union of a tie
//   lane      a two-pointer merge over the two lists, three times at most and with no private array: the union's size; its hash and the
//             content lookup; the ids written
//   wave      no sort and no LDS: lanes take 64 ids of one list at a time and binary-search the other. a[i] lands at i + lower_bound_b(a[i]) -
//             (common ids before i), b[j] at j + lower_bound_a(b[j]) - (common ids before j) unless it is in a; "common ids before" is a ballot
//             prefix popcount plus a running count over the chunks. The counting pass over a gives the exact size, the writing pass scatters
// A winner whose ids lie in a candidate's arena is that list merged with the EMPTY list (nb = 0): the same kernels copy it, the searches in
// the other list cost nothing and there is no pass over b.
#include <hip/hip_runtime.h>

#include "pair_stage.hpp"

namespace pa {
namespace {

// what the rule says of an item without looking at its ids
struct Verdict {
    bool ms, mr;     // the candidates are mapped
    bool tie;        // both mapped, equal keys
    bool r_wins;     // (no tie) the result is R
};
__device__ __forceinline__ Verdict verdict_of(const pa_read_result& s, const pa_read_result& r) {
    Verdict v;
    v.ms = s.mismatches & PA_MAPPED_BIT;
    v.mr = r.mismatches & PA_MAPPED_BIT;
    v.tie = false;
    v.r_wins = !v.ms;
    if (v.ms && v.mr) {   // keys (class non-empty, coverage, -mismatches), compared lexicographically
        const bool es = s.class_len != 0, er = r.class_len != 0;
        if (es != er) v.r_wins = er;
        else if (s.coverage != r.coverage) v.r_wins = r.coverage > s.coverage;
        else if (s.mismatches != r.mismatches) v.r_wins = r.mismatches < s.mismatches;
        else v.tie = true;
    }
    return v;
}

// f(id) for every id of the union of a[0, na) and b[0, nb), ascending, once
template <class F>
__device__ __forceinline__ void for_union(const uint32_t* __restrict__ a, uint32_t na, const uint32_t* __restrict__ b, uint32_t nb, F&& f) {
    uint32_t i = 0, j = 0;
    while (i < na || j < nb) {
        const uint32_t x = i < na ? a[i] : 0, y = j < nb ? b[j] : 0;
        const bool ta = j >= nb || (i < na && x <= y), tb = i >= na || (j < nb && y <= x);   // (both: an id of both lists)
        f(ta ? x : y);
        i += ta;
        j += tb;
    }
}

}  // namespace

// stats: slot 5 = ties. A result is never empty: it has the winner's ids (at least one: an empty winner is final at classify) or a union's
struct StrandRule {
    static constexpr uint32_t LANE_MAX = 32;   // work key (ids to walk over) up to this: a lane; more: a wave
    static constexpr const char* NOUN = "items";
    static constexpr uint32_t ST_TIES = 5, CLASSIFY_STAT = ST_TIES, EMPTY_STAT = NO_STAT;

    static __device__ __forceinline__ Classified classify(const pa_read_result& s, const pa_read_result& r, uint32_t nc) {
        const Verdict v = verdict_of(s, r);
        Classified c{{0, 0, 0, 0}, 0, nc + 2, v.ms, v.mr, v.tie, false};
        pa_read_result& o = c.rec;
        if (v.ms || v.mr) {
            const pa_read_result w = (v.tie || !v.r_wins) ? s : r;   // the winner; on a tie coverage and mismatches are common
            o.coverage = w.coverage;
            o.mismatches = w.mismatches;
            if (w.class_len == 0) c.slot = nc + 1;   // (a tie with an empty S has an empty R: the key's first entry)
            else if ((w.class_off & PA_CLASS_REF) && (!v.tie || r.class_off == w.class_off)) { o.class_off = w.class_off; o.class_len = w.class_len; c.slot = w.class_off & ~PA_CLASS_REF; c.by_ref = true; }
            else c.key = v.tie ? s.class_len + r.class_len : w.class_len;
        }
        return c;
    }

    static __device__ __forceinline__ uint32_t need(const pa_read_result& s, const pa_read_result& r) {
        const bool ms = s.mismatches & PA_MAPPED_BIT, mr = r.mismatches & PA_MAPPED_BIT;
        return (ms ? s.class_len : 0) + (mr ? r.class_len : 0);
    }

    // a tie's two lists, or the winner's list and an empty one
    static __device__ __forceinline__ IdLists lists_of(const PairParams& p, uint32_t item) {
        const pa_read_result s = p.res1[item], r = p.res2[item];
        const Verdict v = verdict_of(s, r);
        const pa_read_result x = (v.tie || !v.r_wins) ? s : r;
        IdLists l{ids_of(x, (v.tie || !v.r_wins) ? p.arena1 : p.arena2, p.ix), nullptr, x.class_len, 0, ref_class_of(x), NO_CLASS};
        l.b = l.a;
        if (v.tie) {
            l.b = ids_of(r, p.arena2, p.ix);
            l.nb = r.class_len;
            l.b_class = ref_class_of(r);
        }
        return l;
    }

    struct Each {   // the union of the two lists
        IdLists l;
        template <class F>
        __device__ __forceinline__ void operator()(F&& f) const { for_union(l.a, l.na, l.b, l.nb, f); }
    };
    static __device__ __forceinline__ Each lane_combine(const IdLists& l, uint32_t& m) {
        uint32_t n = 0;
        for_union(l.a, l.na, l.b, l.nb, [&](uint32_t) { ++n; });
        m = n;   // (m == na: b adds nothing to a)
        return Each{l};
    }

    static __device__ __forceinline__ uint32_t wave_count(const IdLists& l, uint32_t lane) {
        uint32_t common = 0;
        for (uint32_t t0 = 0; t0 < l.na && l.nb != 0; t0 += 64) {   // first pass: how many ids of a are in b too
            const uint32_t t = t0 + lane;
            bool hit = false;
            if (t < l.na) {
                const uint32_t a = l.a[t];
                const uint32_t q = lower_bound_ids(l.b, 0, l.nb, a);
                hit = q < l.nb && l.b[q] == a;
            }
            common += (uint32_t)__popcll(__ballot(hit));
        }
        return l.na + l.nb - common;   // (at least na, which is at least 1)
    }
    static __device__ __forceinline__ void wave_write(const IdLists& l, uint32_t lane, uint32_t* out, uint32_t m) {
        const unsigned long long below = (1ull << lane) - 1;
        uint32_t before = 0;   // ids of both lists in the chunks done
        for (uint32_t t0 = 0; t0 < l.na; t0 += 64) {   // every id of a to its place in the union
            const uint32_t t = t0 + lane;
            bool hit = false;
            uint32_t a = 0, q = 0;
            if (t < l.na) {
                a = l.a[t];
                q = lower_bound_ids(l.b, 0, l.nb, a);
                hit = q < l.nb && l.b[q] == a;
            }
            const unsigned long long mask = __ballot(hit);
            const uint32_t at_a = t + q - (before + (uint32_t)__popcll(mask & below));
            if (t < l.na && at_a < m) out[at_a] = a;   // (at_a < m holds for ascending lists; lists that are not must not write outside)
            before += (uint32_t)__popcll(mask);
        }
        before = 0;
        for (uint32_t t0 = 0; t0 < l.nb; t0 += 64) {   // every id of b that is not in a to its place
            const uint32_t t = t0 + lane;
            bool hit = false;
            uint32_t b = 0, q = 0;
            if (t < l.nb) {
                b = l.b[t];
                q = lower_bound_ids(l.a, 0, l.na, b);
                hit = q < l.na && l.a[q] == b;
            }
            const unsigned long long mask = __ballot(hit);
            const uint32_t at_b = t + q - (before + (uint32_t)__popcll(mask & below));
            if (t < l.nb && !hit && at_b < m) out[at_b] = b;
            before += (uint32_t)__popcll(mask);
        }
    }
};

}  // namespace pa

using namespace pa;

extern "C" size_t pa_strands_scratch_bytes(uint64_t n) { return stage_scratch_bytes(n); }

extern "C" int pa_strands_merge_device(pa_index* idx, const pa_read_result* d_resS, const uint32_t* d_arenaS, const pa_read_result* d_resR, const uint32_t* d_arenaR,
                                       uint64_t n, pa_read_result* d_results, uint32_t* d_arena, uint64_t arena_cap, uint64_t* d_counts, void* d_scratch, size_t scratch_bytes,
                                       void* stream) {
    return stage_launch<StrandRule>(idx, d_resS, d_arenaS, d_resR, d_arenaR, n, d_results, d_arena, arena_cap, d_counts, d_scratch, scratch_bytes, stream);
}

int pa::strands_arena_bound(pa_index* idx, const pa_read_result* d_resS, const pa_read_result* d_resR, uint64_t n, void* d_scratch, void* stream, uint64_t* bound) {
    return stage_arena_bound<StrandRule>(idx, d_resS, d_resR, n, d_scratch, stream, bound);
}

extern "C" int pa_strands_finish(pa_index* idx, void* d_scratch, void* stream, uint64_t stats[PA_STRAND_STATS], uint64_t* arena_used, uint64_t* arena_needed) {
    return stage_finish(idx, d_scratch, stream, stats, arena_used, arena_needed, "strand");
}
