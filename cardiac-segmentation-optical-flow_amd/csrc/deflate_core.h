// DEFLATE (RFC 1951) of one chunk and the CRC-32 arithmetic, as plain C++ shared by the device kernels (csrc/deflate.hip) and a host
// program that runs the very same text on one thread against zlib (tools/deflate_hostcheck.cpp).  Every function is a template on an
// execution context X: X::tid() / X::nt() name the caller among the nt() callers that run the function together, X::sync() is their
// barrier, X::amax / aadd / aor are an integer max, add and bitwise OR on memory they share.  All three commute, every phase between two
// barriers either writes disjoint places or uses only those three, and no phase's work depends on nt(): the bytes that come out are the
// same for 256 device threads as for the host's single one, and the same on every run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ inline
#else
#define DF_HD inline
#endif

namespace cf {
namespace dfl {

constexpr int CH = 32768;          // bytes per chunk: no distance can leave the window, and the chunk fits one stored block
constexpr int SLAB = 256;          // positions whose hash candidates are read together, before any of them enters the heads
constexpr int HBITS = 12;          // hash heads: 4096 ints
constexpr int PBLK = 256;          // positions per parse block
constexpr int MRANGE = 132;        // consecutive positions one caller matches (33 words: neighbouring callers sit in different LDS banks)
constexpr int MINM = 4, MAXM = 258;
constexpr int NLL = 286, ND = 30, NCL = 19;
constexpr int BUF_PAD = 16;        // zero bytes behind the chunk: the word reads of the match loop may look up to 11 bytes past it
constexpr int SLOT = CH + 64;      // bytes of a chunk's output slot (len + 5 at the most are used)

// ---- CRC-32 (zlib's: reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF) as arithmetic in GF(2)[x] mod P(x); bit 31 is x^0
constexpr uint32_t CRC_POLY = 0xEDB88320u;
DF_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P: the operator "append n zero bytes" on a CRC register is gf_mul by it
DF_HD uint32_t gf_xpow8(uint64_t n) {
    uint32_t sq = 1u << 30, p = 1u << 31;       // x^1, x^0
    n *= 8;                                     // n < 2^60
    while (n) {
        if (n & 1u) p = gf_mul(sq, p);
        sq = gf_mul(sq, sq);
        n >>= 1;
    }
    return p;
}
DF_HD uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ CRC_POLY : i >> 1;
    return i;
}

// ---- symbols
DF_HD int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }
// length 3..258 -> code 0..28 (symbol 257 + code), number of extra bits, their value
DF_HD void len_code(int l, int& code, int& nb, int& ex) {
    if (l == 258) { code = 28; nb = 0; ex = 0; return; }
    const int v = l - 3;
    if (v < 8) { code = v; nb = 0; ex = 0; return; }
    nb = ilog2((uint32_t)v) - 2;
    code = 4 * nb + 4 + ((v >> nb) & 3);
    ex = v & ((1 << nb) - 1);
}
// distance 1..32768 -> code 0..29
DF_HD void dist_code(int d, int& code, int& nb, int& ex) {
    const int v = d - 1;
    if (v < 4) { code = v; nb = 0; ex = 0; return; }
    nb = ilog2((uint32_t)v) - 1;
    code = 2 * nb + 2 + ((v >> nb) & 1);
    ex = v & ((1 << nb) - 1);
}
DF_HD uint32_t bit_reverse(uint32_t c, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (c & 1u); c >>= 1; }
    return r;
}

// ---- the small tables of one chunk (2-byte and 4-byte members first: the struct is carved from a 16-byte aligned base)
struct Small {
    uint32_t freq_ll[288], freq_d[32], freq_cl[32];
    uint32_t node_freq[288];           // Huffman build: weights of the internal nodes
    uint32_t part[1024];               // per-caller bit totals -> exclusive bit offsets
    uint32_t flag[CH / 32];            // token starts of the parse
    uint32_t count[32];                // codes per length
    uint32_t next_code[32];
    uint32_t var[16];
    uint16_t code_ll[288], code_d[32], code_cl[32];
    uint16_t order[288];               // used symbols by ascending (weight, symbol)
    uint16_t parent[576];
    uint16_t entry[CH / PBLK];
    uint16_t seq[320];                 // run-length coded code lengths: symbol | extra << 8
    uint8_t len_ll[288], len_d[32], len_cl[32];
};
enum { V_NUSED = 0, V_HLIT, V_HDIST, V_HCLEN, V_NSEQ, V_HDRBITS, V_TOTAL, V_STORED, V_SIZE };

struct State {
    uint8_t* buf;        // [CH + BUF_PAD]  the chunk, zero padded
    uint8_t* step;       // [CH]            0 = literal, else match length - 3
    uint32_t* big;       // [CH / 2]        64 KiB: hash heads, then the parse's exit table (uint16 [CH]), then the output words
    uint32_t* m;         // [CH]            per position: hash candidate + 1, then the match distance (need not be fast memory)
    Small* s;
};

DF_HD uint32_t rd32(const uint8_t* buf, int p) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(buf);
    const uint32_t a = w[p >> 2], b = w[(p >> 2) + 1];
    const int sh = (p & 3) * 8;
    return sh ? (a >> sh) | (b << (32 - sh)) : a;
}
DF_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HBITS); }

// bytes from p that equal the bytes from q < p, at most maxl, of which the first `known` are known to be equal (the sources overlap
// freely: nothing is copied)
DF_HD int match_len(const uint8_t* buf, int p, int q, int maxl, int known) {
    int l = known;
    while (l + 4 <= maxl) {
        const uint32_t x = rd32(buf, p + l) ^ rd32(buf, q + l);
        if (x) return l + (__builtin_ctz(x) >> 3);
        l += 4;
    }
    while (l < maxl && buf[p + l] == buf[q + l]) ++l;
    return l;
}

template <class X>
DF_HD void put_bits(X& x, uint32_t* w, uint32_t pos, uint32_t v, int nbits) {
    if (nbits == 0) return;
    const uint64_t y = (uint64_t)v << (pos & 31);
    x.aor(&w[pos >> 5], (uint32_t)y);
    if (y >> 32) x.aor(&w[(pos >> 5) + 1], (uint32_t)(y >> 32));
}

// Code lengths of at most maxbits for n symbol weights; symbols of weight 0 get length 0.  Fewer than two used symbols are made two
// (weight 1 to the first unused ones, as zlib does), so every code written here is complete.  Called by all callers together.
template <class X>
DF_HD void build_lengths(X& x, Small& s, uint32_t* freq, int n, int maxbits, uint8_t* lens) {
    const int tid = x.tid(), nt = x.nt();
    if (tid == 0) {
        int used = 0;
        for (int i = 0; i < n; ++i) used += freq[i] != 0;
        for (int i = 0; used < 2 && i < n; ++i)
            if (freq[i] == 0) { freq[i] = 1; ++used; }
        s.var[V_NUSED] = (uint32_t)used;
        for (int i = 0; i < 32; ++i) s.count[i] = 0;
    }
    for (int i = tid; i < n; i += nt) lens[i] = 0;
    x.sync();
    const int nu = (int)s.var[V_NUSED];
    // rank sort: ascending weight, ties by symbol
    for (int i = tid; i < n; i += nt) {
        const uint32_t f = freq[i];
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            r += (g != 0) && (g < f || (g == f && j < i));
        }
        s.order[r] = (uint16_t)i;
    }
    x.sync();
    // two-queue Huffman: nodes 0..nu-1 are the sorted leaves, nu..2nu-2 the internal nodes in order of creation (ascending weight)
    if (tid == 0) {
        int i = 0, j = nu;
        for (int k = nu; k < 2 * nu - 1; ++k) {
            uint32_t w = 0;
            for (int t = 0; t < 2; ++t) {
                const bool leaf = i < nu && (j >= k || freq[s.order[i]] <= s.node_freq[j - nu]);
                if (leaf) { w += freq[s.order[i]]; s.parent[i++] = (uint16_t)k; }
                else { w += s.node_freq[j - nu]; s.parent[j++] = (uint16_t)k; }
            }
            s.node_freq[k - nu] = w;
        }
    }
    x.sync();
    for (int i = tid; i < nu; i += nt) {
        int d = 0;
        for (int k = i; k != 2 * nu - 2; k = s.parent[k]) ++d;
        x.aadd(&s.count[d < maxbits ? d : maxbits], 1u);
    }
    x.sync();
    if (tid == 0) {
        // restore the Kraft sum after the fold to maxbits: one code of the deepest level up, one shorter code split in two
        uint32_t total = 0;
        for (int b = maxbits; b > 0; --b) total += s.count[b] << (maxbits - b);
        while (total > (1u << maxbits)) {
            --s.count[maxbits];
            for (int b = maxbits - 1; b > 0; --b)
                if (s.count[b]) { --s.count[b]; s.count[b + 1] += 2; break; }
            --total;
        }
        int j = nu;                                        // the heaviest symbols take the shortest codes
        for (int b = 1; b <= maxbits; ++b)
            for (uint32_t c = s.count[b]; c > 0; --c) lens[s.order[--j]] = (uint8_t)b;
    }
    x.sync();
}

// canonical codes of RFC 1951 3.2.2, stored bit-reversed: the packer writes from the least significant bit
template <class X>
DF_HD void assign_codes(X& x, Small& s, const uint8_t* lens, int n, uint16_t* codes) {
    const int tid = x.tid(), nt = x.nt();
    if (tid == 0) {
        for (int b = 0; b < 16; ++b) s.count[b] = 0;
        for (int i = 0; i < n; ++i) ++s.count[lens[i]];
        s.count[0] = 0;
        uint32_t code = 0;
        for (int b = 1; b < 16; ++b) {
            code = (code + s.count[b - 1]) << 1;
            s.next_code[b] = code;
        }
    }
    x.sync();
    for (int i = tid; i < n; i += nt) {
        const int l = lens[i];
        if (!l) { codes[i] = 0; continue; }
        uint32_t c = s.next_code[l];
        for (int j = 0; j < i; ++j) c += lens[j] == l;
        codes[i] = (uint16_t)bit_reverse(c, l);
    }
    x.sync();
}

DF_HD int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// Bits of the token that starts at p (a literal, or a length / distance pair)
DF_HD uint32_t token_bits(const State& st, int p) {
    const Small& s = *st.s;
    const int b = st.step[p];
    if (!b) return s.len_ll[st.buf[p]];
    int lc, lnb, lex, dc, dnb, dex;
    len_code(b + 3, lc, lnb, lex);
    dist_code((int)st.m[p], dc, dnb, dex);
    return (uint32_t)(s.len_ll[257 + lc] + lnb + s.len_d[dc] + dnb);
}

// One chunk: src[0..len) with 1 <= len <= CH -> slot (SLOT bytes of 4-byte aligned memory), *slot_size = bytes used (<= len + 5).
// The result is one or two non-final blocks that end on a byte boundary: a dynamic-Huffman block followed by an empty stored block (a
// sync flush), or, when that is not smaller, the chunk as a stored block.
template <class X>
DF_HD void compress_chunk(X& x, const uint8_t* src, int len, State& st, uint8_t* slot, int* slot_size) {
    const int tid = x.tid(), nt = x.nt();
    Small& s = *st.s;
    uint8_t* buf = st.buf;
    int* head = reinterpret_cast<int*>(st.big);
    uint16_t* exitp = reinterpret_cast<uint16_t*>(st.big);
    uint32_t* outw = st.big;

    // ---- load, clear
    if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {                      // the usual case: whole words, coalesced
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
        uint32_t* bufw = reinterpret_cast<uint32_t*>(buf);
        for (int i = tid; i < (CH + BUF_PAD) / 4; i += nt) {
            uint32_t w = 0;
            if (4 * i + 4 <= len) w = srcw[i];
            else for (int b = 4 * i; b < len; ++b) w |= (uint32_t)src[b] << (8 * (b - 4 * i));      // the last one to three bytes
            bufw[i] = w;
        }
    } else {
        for (int i = tid; i < CH + BUF_PAD; i += nt) buf[i] = i < len ? src[i] : 0;
    }
    for (int i = tid; i < (1 << HBITS); i += nt) head[i] = 0;
    for (int i = tid; i < 288; i += nt) s.freq_ll[i] = 0;
    for (int i = tid; i < 32; i += nt) { s.freq_d[i] = 0; s.freq_cl[i] = 0; }
    x.sync();

    // ---- hash candidates, slab by slab: a position sees the latest earlier-slab position with its hash (max commutes)
    for (int base = 0; base < len; base += SLAB) {
        for (int i = tid; i < SLAB; i += nt) {
            const int p = base + i;
            if (p < len) st.m[p] = p + MINM <= len ? (uint32_t)head[hash4(rd32(buf, p))] : 0u;
        }
        x.sync();
        for (int i = tid; i < SLAB; i += nt) {
            const int p = base + i;
            if (p + MINM <= len) x.amax(&head[hash4(rd32(buf, p))], p + 1);
        }
        x.sync();
    }

    // ---- longest match per position among the hash candidate and the distances 1, 2, 4, 8 (the previous element of every dtype, which a
    // slab cannot find inside itself); ties go to the distance tried first.  A caller takes MRANGE consecutive positions: a match of l
    // bytes at distance d from p - 1 is one of at least l - 1 bytes at d from p, so inside a run only the new tail is compared (a chunk
    // of zeros costs one word per position and distance instead of 258 bytes), and a candidate is not looked at once an earlier one has
    // reached the longest length possible (inside a long run the hash candidate moves with every position and would be compared from
    // its first byte each time).  The lengths and distances are the exact ones either way.
    for (int v = tid; v * MRANGE < len; v += nt) {
        const int lo = v * MRANGE, hi = lo + MRANGE < len ? lo + MRANGE : len;
        int known[5] = {0, 0, 0, 0, 0}, prev_hd = 0;
        for (int p = lo; p < hi; ++p) {
            const int maxl = len - p < MAXM ? len - p : MAXM;
            const int cand = (int)st.m[p], hd = cand ? p - (cand - 1) : 0;
            int bl = 0, bd = 0;
            const uint32_t here = rd32(buf, p);
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int d = t < 4 ? (1 << t) : hd;
                int k = (t < 4 || hd == prev_hd) ? known[t] - 1 : 0;
                known[t] = 0;
                if (maxl < MINM || d <= 0 || d > p || bl == maxl) continue;   // (nothing beats a full-length match: ties go to the first)
                if (k < MINM) {
                    if (rd32(buf, p - d) != here) continue;
                    k = MINM;
                }
                const int l = match_len(buf, p, p - d, maxl, k < maxl ? k : maxl);
                known[t] = l;
                if (l > bl) { bl = l; bd = d; }
            }
            prev_hd = hd;
            if (bl >= MINM) { st.step[p] = (uint8_t)(bl - 3); st.m[p] = (uint32_t)bd; }
            else st.step[p] = 0;
        }
    }
    x.sync();

    // ---- greedy parse, exact, in three short walks instead of one long one: (a) per block of PBLK positions and per entry position, where
    // the walk leaves the block (backwards, one caller per block); (b) one caller hops block to block from position 0 and notes where each
    // block is entered; (c) every block is walked from its entry and the token starts are flagged.  A walk of len steps becomes
    // PBLK + len / PBLK + PBLK dependent steps.
    const int nblk = (len + PBLK - 1) / PBLK;
    for (int b = tid; b < nblk; b += nt) {
        const int lo = b * PBLK, end = lo + PBLK < len ? lo + PBLK : len;
        for (int p = end - 1; p >= lo; --p) {
            const int sp = st.step[p], nx = p + (sp ? sp + 3 : 1);
            exitp[p] = (uint16_t)(nx >= end ? nx : exitp[nx]);
        }
        s.entry[b] = 0xFFFF;
        for (int i = 0; i < PBLK / 32; ++i) s.flag[b * (PBLK / 32) + i] = 0;
    }
    x.sync();
    if (tid == 0)
        for (int p = 0; p < len; p = exitp[p]) s.entry[p / PBLK] = (uint16_t)p;
    x.sync();
    for (int b = tid; b < nblk; b += nt) {
        const int lo = b * PBLK, end = lo + PBLK < len ? lo + PBLK : len;
        int p = s.entry[b];
        if (p == 0xFFFF) continue;
        while (p < end) {
            s.flag[p >> 5] |= 1u << (p & 31);                 // the block's eight words belong to this caller alone
            const int sp = st.step[p];
            p += sp ? sp + 3 : 1;
        }
    }
    x.sync();

    // ---- histograms (additions commute)
    for (int p = tid; p < len; p += nt) {
        if (!((s.flag[p >> 5] >> (p & 31)) & 1u)) continue;
        const int b = st.step[p];
        if (!b) { x.aadd(&s.freq_ll[buf[p]], 1u); continue; }
        int c, nb, ex;
        len_code(b + 3, c, nb, ex);
        x.aadd(&s.freq_ll[257 + c], 1u);
        dist_code((int)st.m[p], c, nb, ex);
        x.aadd(&s.freq_d[c], 1u);
    }
    if (tid == 0) s.freq_ll[256] = 1;
    x.sync();

    // ---- code lengths and codes
    build_lengths(x, s, s.freq_ll, NLL, 15, s.len_ll);
    build_lengths(x, s, s.freq_d, ND, 15, s.len_d);
    if (tid == 0) {
        int hlit = NLL, hdist = ND;
        while (hlit > 257 && !s.len_ll[hlit - 1]) --hlit;
        while (hdist > 1 && !s.len_d[hdist - 1]) --hdist;
        // run-length code the hlit + hdist lengths as one sequence (runs may cross from one table into the other)
        const int total = hlit + hdist;
        int nseq = 0, i = 0;
        while (i < total) {
            const int v = i < hlit ? s.len_ll[i] : s.len_d[i - hlit];
            int run = 1;
            while (i + run < total && (i + run < hlit ? s.len_ll[i + run] : s.len_d[i + run - hlit]) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int k = run < 138 ? run : 138; s.seq[nseq++] = (uint16_t)(18 | (k - 11) << 8); run -= k; }
                if (run >= 3) { s.seq[nseq++] = (uint16_t)(17 | (run - 3) << 8); run = 0; }
                while (run-- > 0) s.seq[nseq++] = 0;
            } else {
                s.seq[nseq++] = (uint16_t)v; --run;
                while (run >= 3) { const int k = run < 6 ? run : 6; s.seq[nseq++] = (uint16_t)(16 | (k - 3) << 8); run -= k; }
                while (run-- > 0) s.seq[nseq++] = (uint16_t)v;
            }
        }
        for (int k = 0; k < nseq; ++k) ++s.freq_cl[s.seq[k] & 0xFF];
        s.var[V_HLIT] = (uint32_t)hlit; s.var[V_HDIST] = (uint32_t)hdist; s.var[V_NSEQ] = (uint32_t)nseq;
    }
    x.sync();
    build_lengths(x, s, s.freq_cl, NCL, 7, s.len_cl);
    assign_codes(x, s, s.len_ll, NLL, s.code_ll);
    assign_codes(x, s, s.len_d, ND, s.code_d);
    assign_codes(x, s, s.len_cl, NCL, s.code_cl);

    // ---- bit offsets: caller t owns the positions [t R, (t + 1) R); totals, an exclusive scan, then each walks its own range
    const int R = CH / nt;
    const int r0 = tid * R < len ? tid * R : len, r1 = r0 + R < len ? r0 + R : len;
    {
        uint32_t bits = 0;
        for (int p = r0; p < r1; ++p)
            if ((s.flag[p >> 5] >> (p & 31)) & 1u) bits += token_bits(st, p);
        s.part[tid] = bits;
    }
    x.sync();
    const uint8_t perm[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (tid == 0) {
        int hclen = NCL;
        while (hclen > 4 && !s.len_cl[perm[hclen - 1]]) --hclen;
        uint32_t hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
        const int nseq = (int)s.var[V_NSEQ];
        for (int k = 0; k < nseq; ++k) { const int sym = s.seq[k] & 0xFF; hdr += s.len_cl[sym] + cl_extra_bits(sym); }
        uint32_t run = hdr;
        for (int t = 0; t < nt; ++t) { const uint32_t b = s.part[t]; s.part[t] = run; run += b; }
        run += s.len_ll[256];
        const uint32_t bytes = (run + 3 + 7) / 8 + 4;          // + the empty stored block: 3 header bits, padding, 00 00 FF FF
        s.var[V_HCLEN] = (uint32_t)hclen; s.var[V_HDRBITS] = hdr; s.var[V_TOTAL] = run;
        s.var[V_STORED] = bytes >= (uint32_t)len + 5;
        s.var[V_SIZE] = s.var[V_STORED] ? (uint32_t)len + 5 : bytes;
        *slot_size = (int)s.var[V_SIZE];
    }
    x.sync();

    if (s.var[V_STORED]) {
        if (tid == 0) {
            slot[0] = 0;                                       // BFINAL 0, BTYPE 00, padding
            slot[1] = (uint8_t)(len & 0xFF); slot[2] = (uint8_t)(len >> 8);
            slot[3] = (uint8_t)(~len & 0xFF); slot[4] = (uint8_t)((~len >> 8) & 0xFF);
        }
        for (int i = tid; i < len; i += nt) slot[5 + i] = buf[i];
        x.sync();
        return;
    }

    // ---- bits: OR into zeroed words (OR commutes), then the words go to the slot
    const int size = (int)s.var[V_SIZE], nwords = (size + 3) / 4;
    for (int i = tid; i < nwords + 1; i += nt) outw[i] = 0;
    x.sync();
    if (tid == 0) {
        uint32_t pos = 0;
        put_bits(x, outw, pos, 4u, 3); pos += 3;               // BFINAL 0, BTYPE 10
        put_bits(x, outw, pos, s.var[V_HLIT] - 257, 5); pos += 5;
        put_bits(x, outw, pos, s.var[V_HDIST] - 1, 5); pos += 5;
        const int hclen = (int)s.var[V_HCLEN];
        put_bits(x, outw, pos, (uint32_t)hclen - 4, 4); pos += 4;
        for (int k = 0; k < hclen; ++k) { put_bits(x, outw, pos, s.len_cl[perm[k]], 3); pos += 3; }
        const int nseq = (int)s.var[V_NSEQ];
        for (int k = 0; k < nseq; ++k) {
            const int sym = s.seq[k] & 0xFF, ex = s.seq[k] >> 8;
            put_bits(x, outw, pos, s.code_cl[sym], s.len_cl[sym]); pos += s.len_cl[sym];
            put_bits(x, outw, pos, (uint32_t)ex, cl_extra_bits(sym)); pos += cl_extra_bits(sym);
        }
        const uint32_t eob = s.var[V_TOTAL] - s.len_ll[256];
        put_bits(x, outw, eob, s.code_ll[256], s.len_ll[256]);
        const uint32_t b = (s.var[V_TOTAL] + 3 + 7) / 8;       // the empty stored block's LEN / NLEN
        put_bits(x, outw, (b + 2) * 8, 0xFFFFu, 16);
    }
    {
        uint32_t pos = s.part[tid];
        for (int p = r0; p < r1; ++p) {
            if (!((s.flag[p >> 5] >> (p & 31)) & 1u)) continue;
            const int b = st.step[p];
            if (!b) {
                const int c = buf[p];
                put_bits(x, outw, pos, s.code_ll[c], s.len_ll[c]); pos += s.len_ll[c];
                continue;
            }
            int lc, lnb, lex, dc, dnb, dex;
            len_code(b + 3, lc, lnb, lex);
            dist_code((int)st.m[p], dc, dnb, dex);
            const int ll = s.len_ll[257 + lc], dl = s.len_d[dc];
            put_bits(x, outw, pos, (uint32_t)s.code_ll[257 + lc] | (uint32_t)lex << ll, ll + lnb); pos += ll + lnb;
            put_bits(x, outw, pos, (uint32_t)s.code_d[dc] | (uint32_t)dex << dl, dl + dnb); pos += dl + dnb;
        }
    }
    x.sync();
    uint32_t* slotw = reinterpret_cast<uint32_t*>(slot);
    for (int i = tid; i < nwords; i += nt) slotw[i] = outw[i];
    x.sync();
}

}  // namespace dfl
}  // namespace cf
