// DEFLATE (RFC 1951) of one BGZF member, written once for the GPU and for the host: csrc/inflate.hip instantiates inflate_member() with one
// wave as the "lanes", tests/inflate/inflate_host_check.cpp with one scalar lane under ASan + UBSan. No wave intrinsic lives here: what the
// lanes do together (barrier, XOR reduction, staging the payload window) comes in through the Env type.
//
// Env provides
//   uint32_t lane() / lanes()      this lane and how many there are (64 / 1)
//   void     sync()                barrier + memory ordering among the lanes: LDS and the member's own text
//   uint32_t xor_all(uint32_t)     XOR over the lanes
//   void     stage(win, origin)    win[i] = payload[origin + i] for i in [0, IN_WIN), 0 where origin + i is outside [0, in_len)
//   uint8_t  payload(i)            one payload byte, i < in_len (stored blocks are copied from the payload, not through the window)
//
// How a member runs. Decoding is serial and WAVE-UNIFORM: every lane runs the same bit reader over the same LDS window and holds the same
// state, so no state is ever handed from lane to lane. The decode emits tokens (a literal, or a match of length and distance) into a batch
// in `Work`; the lanes then execute the batch together, byte p of the batch's output by lane p % lanes: the byte's token is found by binary
// search, a match byte is followed to its source (out[p] = out[start - d + (p - start) % d]: periodic when the distance is below the length)
// until the source is a literal of the batch or lies before the batch, i.e. in text that a barrier has already ordered. Each hop lands in an
// earlier token, so a byte takes at most TOK hops. The text is written byte by byte: a member's first and last bytes have no alignment and the
// neighbours are written by other waves at the same time, so nothing wider than the member's own bytes is ever stored.
// History is the text itself (HBM, the member's own 64 KiB: hot in L2); the variant with a 32 KiB LDS ring is in DESIGN.md §8.
//
// What "wave-uniform" relies on: build(), the code-length parse and the token writes are plain read-modify-writes of LDS words executed by all 64 lanes
// with identical operands (h.count[..]++ is one ds_read and one ds_write of the same address and value in every lane). By the letter of the C++ memory
// model that is a race between threads; on the hardware it is one wave executing one instruction stream in lockstep, the LDS keeps a wave's operations in
// program order, and the compiler may not reorder a thread's own accesses to one address. Every lane therefore reads what it wrote itself, which is what
// every other lane wrote too. Data that one lane writes and ANOTHER reads (lookup tables, the staged window, text) always has a sync() in between.
// Worst case of the batch execution, not measured: a run like b"A" * 65536 is a chain of distance-1 matches, so a byte walks back through every earlier
// token of its batch (up to TOK hops of a 7-step binary search in LDS) before it reaches a literal or ordered text; correct and bounded, but far below the
// FASTQ rate. Resolving such chains token by token behind a barrier is the alternative.
//
// Bounds do not rest on the stream: the window reader indexes win[] under a range check, stage()/payload() are bounded by in_len, every
// text store is at p < out_len and every text load at q < p. Every loop consumes at least one bit or produces one byte and ends at in_len /
// out_len, so a corrupt payload ends with a status.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pseudoaligner_amd.h"

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif

namespace pa_inflate {

constexpr uint32_t IN_WIN = 4096;     // bytes of payload staged at a time
constexpr uint32_t IN_AHEAD = 1024;   // staged bytes in front of the reader before each step (a batch reads < 6 * TOK + 16, a dynamic header < 600)
constexpr uint32_t TOK = 128;         // tokens per batch
constexpr uint32_t LIT_LUT_BITS = 10, DIST_LUT_BITS = 8;
constexpr uint32_t CRC_POLY = 0xEDB88320u;

struct Work {
    alignas(16) uint8_t win[IN_WIN];
    uint32_t crc_tab[256];
    uint32_t tok_start[TOK];   // text offset (inside the member) of the token's first byte
    uint16_t tok_len[TOK];     // match length; the byte itself for a literal
    uint16_t tok_dist[TOK];    // 0 = literal
    uint16_t lit_count[16], lit_symbol[288], lit_lut[1u << LIT_LUT_BITS];
    uint16_t dist_count[16], dist_symbol[32], dist_lut[1u << DIST_LUT_BITS];
    uint8_t lens[320];
};

struct Huff {
    uint16_t* count;    // [16] codes per length
    uint16_t* symbol;   // symbols in canonical order
    uint16_t* lut;      // [1 << lut_bits]: (symbol << 4) | length for codes of at most lut_bits bits, 0 = longer or unused
    uint32_t lut_bits;  // 0 = no table
};

struct Reader {
    uint64_t buf;        // unread bits, LSB first
    uint32_t cnt;        // how many
    uint32_t next;       // payload index of the next byte to load
    const uint8_t* win;  // staged payload
    int32_t origin;      // payload index of win[0]: first_origin (<= 0) plus a multiple of 16
    uint32_t in_len;
};

PA_HD void refill(Reader& r) {   // afterwards cnt >= 33; bytes outside the window or the payload read as 0
    while (r.cnt <= 32) {
        const uint32_t w = (uint32_t)((int32_t)r.next - r.origin);
        if ((w & 3u) == 0 && w + 4 <= IN_WIN) {
            uint32_t v;
            memcpy(&v, r.win + w, 4);
            r.buf |= (uint64_t)v << r.cnt;
            r.cnt += 32;
            r.next += 4;
        } else {
            const uint32_t v = w < IN_WIN ? r.win[w] : 0u;
            r.buf |= (uint64_t)v << r.cnt;
            r.cnt += 8;
            r.next += 1;
        }
    }
}
PA_HD void drop(Reader& r, uint32_t n) { r.buf >>= n; r.cnt -= n; }
PA_HD uint32_t take(Reader& r, uint32_t n) {   // n <= 32
    refill(r);
    const uint32_t v = (uint32_t)(r.buf & ((1ull << n) - 1));
    drop(r, n);
    return v;
}
PA_HD uint64_t consumed_bits(const Reader& r) { return (uint64_t)r.next * 8 - r.cnt; }
PA_HD bool exhausted(const Reader& r) { return consumed_bits(r) > (uint64_t)r.in_len * 8; }
PA_HD void seek(Reader& r, uint32_t byte) { r.buf = 0; r.cnt = 0; r.next = byte; }

// canonical walk (one bit per step) over the low `maxbits` bits of `bits`: the symbol and *len, or -1 when no code of at most maxbits bits matches
PA_HD int walk(const Huff& h, uint32_t bits, uint32_t maxbits, uint32_t* len) {
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= maxbits; l++) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int count = h.count[l];
        if (code - count < first) { *len = l; return h.symbol[index + (code - first)]; }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// count[] and symbol[] from n code lengths. Returns what is left of the code space: 0 complete, > 0 incomplete, < 0 over-subscribed; *max_len = longest code
PA_HD int build(const Huff& h, const uint8_t* lens, uint32_t n, uint32_t* max_len) {
    for (uint32_t l = 0; l < 16; l++) h.count[l] = 0;
    for (uint32_t i = 0; i < n; i++) h.count[lens[i] & 15]++;
    int left = 1;
    uint32_t mx = 0;
    for (uint32_t l = 1; l < 16; l++) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
        if (h.count[l]) mx = l;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (uint32_t i = 0; i < n; i++)
        if (lens[i] & 15) h.symbol[offs[lens[i] & 15]++] = (uint16_t)i;
    *max_len = mx;
    return left;
}

// this lane's entries of the lookup table
PA_HD void fill_lut(const Huff& h, uint32_t lane, uint32_t lanes) {
    for (uint32_t e = lane; e < (1u << h.lut_bits); e += lanes) {
        uint32_t len = 0;
        const int s = walk(h, e, h.lut_bits, &len);
        h.lut[e] = s < 0 ? (uint16_t)0 : (uint16_t)(((uint32_t)s << 4) | len);
    }
}

PA_HD int decode_sym(Reader& r, const Huff& h) {   // -1 = no such code
    refill(r);
    if (h.lut_bits) {
        const uint32_t e = h.lut[r.buf & ((1u << h.lut_bits) - 1)];
        if (e) { drop(r, e & 15u); return (int)(e >> 4); }
    }
    uint32_t len = 0;
    const int s = walk(h, (uint32_t)r.buf, 15, &len);
    if (s >= 0) drop(r, len);
    return s;
}

// ---- CRC-32 (zlib's polynomial, reflected) and its combine rule ----
PA_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}
PA_HD uint32_t gf2_mul(uint32_t a, uint32_t b) {   // a(x) b(x) mod P, bit 31 = x^0
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
PA_HD uint32_t gf2_x8n(uint32_t n) {   // x^(8 n) mod P
    uint32_t p = 1u << 31, sq = gf2_mul(gf2_mul(1u << 30, 1u << 30), gf2_mul(1u << 30, 1u << 30));   // x^4
    sq = gf2_mul(sq, sq);                                                                             // x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = gf2_mul(sq, p);
        sq = gf2_mul(sq, sq);
    }
    return p;
}

PA_HD uint32_t finish(const Reader& r, uint32_t code) { return exhausted(r) ? (uint32_t)PA_INFLATE_INPUT_EXHAUSTED : code; }

// the tokens of the batch, executed by this lane: text bytes [batch_start, out_end)
PA_HD void execute_batch(const Work& w, uint32_t ntok, uint32_t batch_start, uint32_t out_end, uint8_t* text, uint32_t lane, uint32_t lanes) {
    for (uint32_t p = batch_start + lane; p < out_end; p += lanes) {
        uint32_t q = p, byte = 0;
        for (uint32_t hop = 0; hop <= TOK; hop++) {
            if (q < batch_start) { byte = text[q]; break; }
            uint32_t lo = 0, hi = ntok;   // the last token that starts at or before q
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (w.tok_start[mid] <= q) lo = mid; else hi = mid;
            }
            const uint32_t d = w.tok_dist[lo];
            if (d == 0) { byte = w.tok_len[lo]; break; }
            q = w.tok_start[lo] - d + (q - w.tok_start[lo]) % d;   // d <= tok_start (checked when the token was made): q < tok_start[lo]
        }
        text[p] = (uint8_t)byte;
    }
}

template <class Env>
PA_HD void restage(Env& env, Work& w, Reader& r) {
    const uint32_t at = (uint32_t)((int32_t)r.next - r.origin);
    if (at + IN_AHEAD <= IN_WIN || (int64_t)r.origin + IN_WIN >= (int64_t)r.in_len) return;   // enough in front, or the window already holds the payload's end
    // (behind a long stored block `at` may lie beyond the window: the move below brings it back to at < 16)
    env.sync();
    r.origin += (int32_t)(at & ~15u);
    env.stage(w.win, r.origin);
    env.sync();
}

// One member: payload of in_len bytes -> text[0, out_len). Returns the status (PA_INFLATE_*); *crc_out = CRC-32 of the text when the status is
// PA_INFLATE_OK or PA_INFLATE_CRC_MISMATCH. first_origin: payload index of win[0] for the first window (<= 0, so that the device can stage whole aligned vectors).
template <class Env>
PA_HD uint32_t inflate_member(Env& env, Work& w, uint32_t in_len, uint8_t* text, uint32_t out_len, uint32_t want_crc, int32_t first_origin, uint32_t* crc_out) {
    const uint32_t lane = env.lane(), lanes = env.lanes();
    const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

    for (uint32_t i = lane; i < 256; i += lanes) w.crc_tab[i] = crc_table_entry(i);
    Reader r;
    r.buf = 0; r.cnt = 0; r.next = 0; r.win = w.win; r.origin = first_origin; r.in_len = in_len;
    env.sync();
    env.stage(w.win, r.origin);
    env.sync();

    const Huff lit = {w.lit_count, w.lit_symbol, w.lit_lut, LIT_LUT_BITS};
    const Huff dist = {w.dist_count, w.dist_symbol, w.dist_lut, DIST_LUT_BITS};
    const Huff clen = {w.dist_count, w.dist_symbol, w.dist_lut, 0};   // the code-length code lives where the distance code will be built afterwards
    uint32_t out = 0, last = 0;

    // every pass of this loop reads at least the three header bits of a block: at most 8 in_len / 3 + 1 passes
    while (!last) {
        restage(env, w, r);
        last = take(r, 1);
        const uint32_t type = take(r, 2);
        if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
        if (type == 3) return PA_INFLATE_BAD_BLOCK_TYPE;
        if (type == 0) {
            drop(r, r.cnt & 7u);   // to the byte boundary
            const uint32_t len = take(r, 16), nlen = take(r, 16);
            if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
            if ((len ^ 0xFFFFu) != nlen) return PA_INFLATE_STORED_LEN;
            const uint32_t from = (uint32_t)(consumed_bits(r) >> 3);   // a whole number of bytes here
            if ((uint64_t)from + len > in_len) return PA_INFLATE_INPUT_EXHAUSTED;
            if (len > out_len - out) return PA_INFLATE_OUTPUT_TOO_LONG;
            for (uint32_t i = lane; i < len; i += lanes) text[out + i] = env.payload(from + i);
            out += len;
            seek(r, from + len);
            env.sync();   // the stored bytes are history for the blocks behind
            continue;
        }
        if (type == 1) {
            for (uint32_t i = 0; i < 288; i++) w.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            for (uint32_t i = 0; i < 32; i++) w.lens[288 + i] = 5;   // 30 and 31 have codes and are refused when met
            uint32_t mx = 0;
            build(lit, w.lens, 288, &mx);
            build(dist, w.lens + 288, 32, &mx);
        } else {
            const uint32_t nlen = take(r, 5) + 257, ndist = take(r, 5) + 1, ncode = take(r, 4) + 4;
            if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
            if (nlen > 286 || ndist > 30) return PA_INFLATE_TOO_MANY_SYMBOLS;
            for (uint32_t i = 0; i < 19; i++) w.lens[i] = 0;
            for (uint32_t i = 0; i < ncode; i++) w.lens[ORDER[i]] = (uint8_t)take(r, 3);
            if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
            uint32_t mx = 0;
            if (build(clen, w.lens, 19, &mx) != 0) return PA_INFLATE_BAD_CODE_LENGTHS;   // zlib: the code-length code must be complete
            uint32_t have = 0;
            while (have < nlen + ndist) {   // each pass adds at least one length
                const int s = decode_sym(r, clen);
                if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
                if (s < 0) return PA_INFLATE_BAD_CODE_LENGTHS;
                if (s < 16) { w.lens[have++] = (uint8_t)s; continue; }
                uint32_t prev = 0, rep;
                if (s == 16) {
                    if (have == 0) return PA_INFLATE_BAD_REPEAT;
                    prev = w.lens[have - 1];
                    rep = 3 + take(r, 2);
                } else if (s == 17) rep = 3 + take(r, 3);
                else rep = 11 + take(r, 7);
                if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
                if (have + rep > nlen + ndist) return PA_INFLATE_BAD_REPEAT;
                while (rep--) w.lens[have++] = (uint8_t)prev;
            }
            if (w.lens[256] == 0) return PA_INFLATE_NO_END_OF_BLOCK;
            // the distance lengths move out of the way of nothing: lens[nlen ..) is read by build() before the distance arrays are written,
            // but the code-length code shares them, so copy first
            uint8_t dl[32];
            for (uint32_t i = 0; i < ndist; i++) dl[i] = w.lens[nlen + i];
            int left = build(lit, w.lens, nlen, &mx);
            if (left < 0 || (left > 0 && mx != 1)) return PA_INFLATE_BAD_CODE_LENGTHS;   // incomplete only as a single code of one bit
            left = build(dist, dl, ndist, &mx);
            if (left < 0 || (left > 0 && mx > 1)) return PA_INFLATE_BAD_CODE_LENGTHS;    // ... or no distance code at all
        }
        env.sync();
        fill_lut(lit, lane, lanes);
        fill_lut(dist, lane, lanes);
        env.sync();

        // symbols of the block, a batch of tokens at a time
        bool eob = false;
        while (!eob) {
            restage(env, w, r);
            const uint32_t batch_start = out;
            uint32_t ntok = 0, err = 0;
            while (ntok < TOK) {   // each pass consumes at least one bit
                int s = decode_sym(r, lit);
                if (exhausted(r)) { err = PA_INFLATE_INPUT_EXHAUSTED; break; }
                if (s < 0 || s > 285) { err = PA_INFLATE_BAD_SYMBOL; break; }
                if (s == 256) { eob = true; break; }
                if (s < 256) {
                    if (out >= out_len) { err = PA_INFLATE_OUTPUT_TOO_LONG; break; }
                    w.tok_start[ntok] = out; w.tok_len[ntok] = (uint16_t)s; w.tok_dist[ntok] = 0;
                    ntok++;
                    out++;
                    continue;
                }
                s -= 257;
                // RFC 1951 3.2.5 as arithmetic: symbols 257..264 are lengths 3..10, then four symbols per extra bit, 285 is 258 (and 284 + 31 is 258 too)
                const uint32_t le = s < 8 || s == 28 ? 0u : (uint32_t)(s - 4) >> 2;
                const uint32_t len = (s < 8 ? 3u + (uint32_t)s : s == 28 ? 258u : 3u + ((4u + ((uint32_t)s & 3u)) << le)) + take(r, le);
                const int ds = decode_sym(r, dist);
                if (exhausted(r)) { err = PA_INFLATE_INPUT_EXHAUSTED; break; }
                if (ds < 0 || ds > 29) { err = PA_INFLATE_BAD_SYMBOL; break; }
                const uint32_t de = ds < 4 ? 0u : (uint32_t)(ds - 2) >> 1;   // two symbols per extra bit
                const uint32_t d = (ds < 4 ? 1u + (uint32_t)ds : 1u + ((2u + ((uint32_t)ds & 1u)) << de)) + take(r, de);
                if (exhausted(r)) { err = PA_INFLATE_INPUT_EXHAUSTED; break; }
                if (d > out) { err = PA_INFLATE_DISTANCE_TOO_FAR; break; }
                if (len > out_len - out) { err = PA_INFLATE_OUTPUT_TOO_LONG; break; }
                w.tok_start[ntok] = out; w.tok_len[ntok] = (uint16_t)len; w.tok_dist[ntok] = (uint16_t)d;
                ntok++;
                out += len;
            }
            env.sync();
            if (ntok) execute_batch(w, ntok, batch_start, out, text, lane, lanes);   // also in front of an error: the bytes are inside the member either way
            env.sync();
            if (err) return err;
        }
    }
    if (exhausted(r)) return PA_INFLATE_INPUT_EXHAUSTED;
    if ((consumed_bits(r) + 7) / 8 != in_len) return PA_INFLATE_TRAILING_INPUT;
    if (out != out_len) return PA_INFLATE_OUTPUT_TOO_SHORT;

    // CRC-32: the text in 64 contiguous pieces, each shifted by the bytes behind it (crc32_combine's rule), XORed together. Pieces of length 0 add 0
    const uint32_t piece = (out_len + 63) / 64;
    uint32_t acc = 0;
    for (uint32_t k = lane; k < 64; k += lanes) {
        const uint32_t b = k * piece < out_len ? k * piece : out_len, e = b + piece < out_len ? b + piece : out_len;
        if (e == b) continue;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = b; i < e; i++) c = w.crc_tab[(c ^ text[i]) & 0xFFu] ^ (c >> 8);
        c ^= 0xFFFFFFFFu;
        acc ^= gf2_mul(gf2_x8n(out_len - e), c);
    }
    const uint32_t crc = env.xor_all(acc);
    *crc_out = crc;
    return crc == want_crc ? PA_INFLATE_OK : PA_INFLATE_CRC_MISMATCH;
}

}  // namespace pa_inflate
