// Builder and reader of the k <= 32 dictionary (layout: device_layout.hpp; the kernel's own probe is lane_steps.hpp, SEEK).
// One text for the CPU flattener (device_flatten.cpp: threads, __atomic builtins) and the GPU filler (index_fill.hip: atomicCAS /
// atomicAnd): the atomics come in as a policy type. Insertion is two passes over all keys with a barrier in between:
//   pass 1  every key tries its HOME slot only                    (so that as many keys as possible are found by the first load)
//   pass 2  keys that are not in their home slot take another slot of the bucket and leave a flag in the home slot, or go on to the
//           next bucket (overflow flag in the home slot) where the same rule applies
// Nothing is ever removed, so "the home slot names no other slot and no overflow" proves a key absent.
// The pair dictionary (k <= 24) has its own insert, flag pass and lookup below.
#pragma once
#include "lane_steps.hpp"

namespace pa {

// the atomics policy of host threads (the CPU flattener, the tests' host checks)
struct HostAtomics {
    static bool cas(uint32_t* p, uint32_t expect, uint32_t v) { return __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); }
    static void and_(uint32_t* p, uint32_t m) { __atomic_fetch_and(p, m, __ATOMIC_RELAXED); }
    static uint64_t min64(uint64_t* p, uint64_t v) {
        uint64_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
        return old;
    }
    static void and64(uint64_t* p, uint64_t m) { __atomic_fetch_and(p, m, __ATOMIC_RELAXED); }
};

template <class A>
PA_HD bool slot_claim(uint32_t* slot, uint64_t km, uint32_t handle, uint32_t off) {
    if (!A::cas(slot + 2, NO_HANDLE, handle)) return false;
    slot[0] = (uint32_t)km;
    slot[1] = (uint32_t)(km >> 32);
    A::and_(slot + 3, off | ~SLOT_OFF_MASK);   // (other threads may already be clearing flag bits of this word)
    return true;
}

template <class A>
PA_HD void dict_insert_home(uint32_t* table, uint32_t nbuckets, uint64_t km, uint32_t handle, uint32_t off) {
    uint32_t home;
    const uint32_t b = pa_bucket_home(km, nbuckets, home);
    slot_claim<A>(table + (uint64_t)b * BUCKET_WORDS + SLOT_WORDS * home, km, handle, off);
}

template <class A>
PA_HD void dict_insert_rest(uint32_t* table, uint32_t nbuckets, uint64_t km, uint32_t handle, uint32_t off) {
    uint32_t home;
    uint32_t b = pa_bucket_home(km, nbuckets, home);
    {
        const uint32_t* hs = table + (uint64_t)b * BUCKET_WORDS + SLOT_WORDS * home;   // written in pass 1 if at all
        if (hs[2] != NO_HANDLE && hs[0] == (uint32_t)km && hs[1] == (uint32_t)(km >> 32)) return;
    }
    for (bool first = true;; first = false) {   // load <= 1/2 (DICT_LOAD): a free slot exists
        uint32_t* line = table + (uint64_t)b * BUCKET_WORDS;
        uint32_t* hs = line + SLOT_WORDS * home;
        if (!first && slot_claim<A>(hs, km, handle, off)) return;   // (in a later bucket the home slot may be free)
        for (uint32_t i = 0; i < 3; ++i)
            if (slot_claim<A>(line + SLOT_WORDS * ((home + 1 + i) & 3u), km, handle, off)) {
                A::and_(hs + 3, ~(1u << (SLOT_FLAG_SHIFT + i)));
                return;
            }
        A::and_(hs + 3, ~(SLOT_FLAG_OVERFLOW << SLOT_FLAG_SHIFT));
        if (++b == nbuckets) b = 0;
    }
}

// the lookup the kernel performs, as a loop (builders' self-check, edge derivation); `probes` = buckets beyond the first
PA_HD bool dict_find64(const uint32_t* table, uint32_t nbuckets, uint64_t km, uint32_t& handle, uint32_t& off, uint32_t& probes) {
    uint32_t home;
    uint32_t b = pa_bucket_home(km, nbuckets, home);
    const uint32_t klo = (uint32_t)km, khi = (uint32_t)(km >> 32);
    for (probes = 0; probes < nbuckets; ++probes) {
        const uint32_t* line = table + (uint64_t)b * BUCKET_WORDS;
        const U4 v = *reinterpret_cast<const U4*>(line + SLOT_WORDS * home);
        if (slot_holds(v, klo, khi)) { handle = v.z; off = v.w & SLOT_OFF_MASK; return true; }
        const uint32_t fl = slot_flags(v);
        for (uint32_t c = fl & 7u; c; c &= c - 1) {
            const U4 v2 = *reinterpret_cast<const U4*>(line + SLOT_WORDS * ((home + 1 + pa_ctz32(c)) & 3u));
            if (slot_holds(v2, klo, khi)) { handle = v2.z; off = v2.w & SLOT_OFF_MASK; return true; }
        }
        if (!(fl & SLOT_FLAG_OVERFLOW)) return false;
        if (++b == nbuckets) b = 0;
    }
    return false;
}

// ---- the pair dictionary (device_layout.hpp). The policy type also brings 64-bit atomics: min64 (returns the word it found) and and64.
// Pass 1, every key: pair_insert. Barrier. Pass 2, every key: pair_flag. The table starts as all ones.

// false: some key (this one, or one it displaced) would lie further from its home than pair_max_disp(b) — the table is too small
template <class A>
PA_HD bool pair_insert(uint64_t* table, uint32_t b, uint64_t km, uint32_t handle, uint32_t off) {
    const uint32_t rbits = PAIR_KEY_BITS - b, mask = (uint32_t)((1ull << b) - 1), maxd = pair_max_disp(b);
    const uint64_t m = pair_mix(km);
    uint32_t p = (uint32_t)(m >> rbits);
    uint64_t w = pair_entry((uint32_t)m & ((1u << rbits) - 1u), handle, off);
    for (;;) {   // the pair keeps the two smallest words it is offered, the larger ones go on
        uint64_t* e = table + 2ull * p;
        uint64_t old = A::min64(e, w);
        if (old > w) w = old;
        if (w == PAIR_EMPTY) return true;
        old = A::min64(e + 1, w);
        if (old > w) w = old;
        if (w == PAIR_EMPTY) return true;
        if ((pair_entry_tag(w) >> rbits) >= maxd) return false;
        w += 1ull << (PAIR_TAG_SHIFT + rbits);   // one pair further from its home
        p = (p + 1) & mask;
    }
}

// where the key lies (pairs from home), or NO_HANDLE
PA_HD uint32_t pair_locate(const uint64_t* table, uint32_t b, uint64_t km, uint64_t& entry) {
    const uint32_t rbits = PAIR_KEY_BITS - b, mask = (uint32_t)((1ull << b) - 1), maxd = pair_max_disp(b);
    const uint64_t m = pair_mix(km);
    const uint32_t q = (uint32_t)(m >> rbits), r = (uint32_t)m & ((1u << rbits) - 1u);
    for (uint32_t d = 0; d <= maxd; ++d) {
        const uint64_t* e = table + 2ull * ((q + d) & mask);
        const uint32_t want = r | (d << rbits);
        for (uint32_t i = 0; i < 2; ++i) {
            const uint64_t w = e[i];   // (pass 2 only clears flag bits: the tags stand)
            if (pair_entry_tag(w) == want) { entry = w; return d; }
        }
    }
    return NO_HANDLE;
}

// pass 2: every pair the key came through says that a key lies further on
template <class A>
PA_HD void pair_flag(uint64_t* table, uint32_t b, uint64_t km) {
    uint64_t w;
    const uint32_t d = pair_locate(table, b, km, w);
    if (d == NO_HANDLE || d == 0) return;
    const uint32_t mask = (uint32_t)((1ull << b) - 1), q = (uint32_t)(pair_mix(km) >> (PAIR_KEY_BITS - b));
    for (uint32_t j = 0; j < d; ++j) A::and64(table + 2ull * ((q + j) & mask), ~(1ull << PAIR_FLAG_BIT));
}

// the lookup the kernel performs, as a loop; `probes` = pairs beyond the first
PA_HD bool pair_find64(const uint64_t* table, uint32_t b, uint64_t km, uint32_t& handle, uint32_t& off, uint32_t& probes) {
    const uint32_t rbits = PAIR_KEY_BITS - b, mask = (uint32_t)((1ull << b) - 1), maxd = pair_max_disp(b);
    const uint64_t m = pair_mix(km);
    const uint32_t q = (uint32_t)(m >> rbits), r = (uint32_t)m & ((1u << rbits) - 1u);
    for (probes = 0;; ++probes) {
        const uint64_t* e = table + 2ull * ((q + probes) & mask);
        const uint64_t e0 = e[0], e1 = e[1];
        const uint32_t want = r | (probes << rbits);
        if (pair_entry_tag(e0) == want) { handle = pair_entry_handle(e0); off = pair_entry_off(e0); return true; }
        if (pair_entry_tag(e1) == want) { handle = pair_entry_handle(e1); off = pair_entry_off(e1); return true; }
        if (((e0 >> PAIR_FLAG_BIT) & 1u) || probes >= maxd) return false;
    }
}

// either format: dict_pairs != 0 selects the pair dictionary
PA_HD bool dict_find64(const uint32_t* table, uint32_t nbuckets, uint32_t dict_pairs, uint64_t km, uint32_t& handle, uint32_t& off, uint32_t& probes) {
    if (dict_pairs) return pair_find64(reinterpret_cast<const uint64_t*>(table), dict_pairs, km, handle, off, probes);
    return dict_find64(table, nbuckets, km, handle, off, probes);
}

}  // namespace pa
