// Runs the text of csrc/deflate_core.h -- the chunk compressor and the CRC-32 arithmetic that csrc/deflate.hip runs on the device -- on one
// host thread and holds it to zlib: every stream must inflate (raw, wbits -15) to the bytes it was made from, never exceed len + 5 per
// chunk, and the CRC folded from 1 KiB pieces with the GF(2) operators must equal zlib's crc32.  No GPU is involved: RFC 1951's corners
// (15-bit limit, one or no distance code, run-length coded headers, the stored fallback) are found here first.
//   g++ -O2 -std=c++17 -fsanitize=address,undefined tools/deflate_hostcheck.cpp -lz -o deflate_hostcheck && ./deflate_hostcheck [file ...]
// With file arguments each file is compressed too and its stream is written beside it as <file>.deflate (final block 03 00 appended).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../cardiac-segmentation-optical-flow_amd/csrc/deflate_core.h"

using namespace cf::dfl;

struct HostX {
    int tid() const { return 0; }
    int nt() const { return 1; }
    void sync() const {}
    void amax(int* a, int v) const { if (v > *a) *a = v; }
    void aadd(uint32_t* a, uint32_t v) const { *a += v; }
    void aor(uint32_t* a, uint32_t v) const { *a |= v; }
};

static int failures = 0;

// depth of the unrestricted Huffman tree of a histogram: above 15, the length limit of build_lengths acted on the chunk
static int huffman_depth(const uint32_t* freq, int n) {
    std::vector<std::pair<uint64_t, int>> h;
    for (int i = 0; i < n; ++i) if (freq[i]) h.push_back({freq[i], 0});
    auto cmp = [](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) { return a > b; };
    std::make_heap(h.begin(), h.end(), cmp);
    while (h.size() > 1) {
        std::pop_heap(h.begin(), h.end(), cmp); auto a = h.back(); h.pop_back();
        std::pop_heap(h.begin(), h.end(), cmp); auto b = h.back(); h.pop_back();
        h.push_back({a.first + b.first, std::max(a.second, b.second) + 1});
        std::push_heap(h.begin(), h.end(), cmp);
    }
    return h.empty() ? 0 : h[0].second;
}
static int deepest_ll = 0;          // over the chunks of the last deflate_host call

static std::vector<uint8_t> deflate_host(const std::vector<uint8_t>& src, size_t* worst_over = nullptr) {
    // exact-size allocations, so that the address sanitizer sees every overrun of the chunk state
    std::vector<uint32_t> bufw((CH + BUF_PAD) / 4), big(CH / 2), m(CH), slotw(SLOT / 4);
    std::vector<uint8_t> step(CH);
    std::vector<Small> small(1);
    State st;
    st.buf = reinterpret_cast<uint8_t*>(bufw.data());
    st.step = step.data();
    st.big = big.data();
    st.m = m.data();
    st.s = small.data();
    HostX x;
    std::vector<uint8_t> out;
    deepest_ll = 0;
    for (size_t off = 0; off < src.size(); off += CH) {
        const int len = (int)std::min<size_t>(CH, src.size() - off);
        std::fill(big.begin(), big.end(), 0xFFFFFFFFu);            // the compressor must not rely on what the memory held
        std::fill(m.begin(), m.end(), 0xFFFFFFFFu);
        std::fill(step.begin(), step.end(), 0xFF);
        memset(small.data(), 0xFF, sizeof(Small));
        int size = -1;
        compress_chunk(x, src.data() + off, len, st, reinterpret_cast<uint8_t*>(slotw.data()), &size);
        deepest_ll = std::max(deepest_ll, huffman_depth(small[0].freq_ll, NLL));
        if (size < 1 || size > len + 5) { printf("FAIL: chunk of %d bytes took %d\n", len, size); exit(1); }
        if (worst_over && (size_t)size == (size_t)len + 5) ++*worst_over;
        const uint8_t* s = reinterpret_cast<const uint8_t*>(slotw.data());
        out.insert(out.end(), s, s + size);
    }
    return out;
}

static bool inflate_equals(std::vector<uint8_t> stream, const std::vector<uint8_t>& want) {
    stream.push_back(3); stream.push_back(0);
    std::vector<uint8_t> got(want.size() + 16);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = stream.data(); z.avail_in = (uInt)stream.size();
    z.next_out = got.data(); z.avail_out = (uInt)got.size();
    const int rc = inflate(&z, Z_FINISH);
    const size_t n = z.total_out;
    const bool all_in = z.avail_in == 0;
    inflateEnd(&z);
    if (rc != Z_STREAM_END || n != want.size() || !all_in) { printf("  inflate rc %d, %zu of %zu bytes, msg %s\n", rc, n, want.size(), z.msg ? z.msg : "-"); return false; }
    return n == 0 || memcmp(got.data(), want.data(), n) == 0;
}

// the kernels' CRC: 1 KiB pieces aligned to the end, folded left to right with the shift operator
static uint32_t crc_pieces(const std::vector<uint8_t>& v) {
    const size_t P = 1024, n = v.size();
    if (!n) return 0;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = crc_table_entry(i);
    const size_t np = (n + P - 1) / P, pad = np * P - n;
    const uint32_t xp = gf_xpow8(P);
    uint32_t acc = 0;
    for (size_t g = 0; g < np; ++g) {
        const size_t lo = g * P < pad ? 0 : g * P - pad, hi = (g + 1) * P - pad;
        uint32_t c = 0;
        for (size_t i = lo; i < hi; ++i) c = table[(c ^ v[i]) & 0xFF] ^ (c >> 8);
        acc = gf_mul(xp, acc) ^ c;
    }
    return acc ^ gf_mul(gf_xpow8(n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
}

static void check(const std::string& name, const std::vector<uint8_t>& v) {
    size_t stored = 0;
    const std::vector<uint8_t> s = deflate_host(v, &stored);
    const bool ok = inflate_equals(s, v);
    const uint32_t c = crc_pieces(v), zc = (uint32_t)crc32(0L, v.data(), (uInt)v.size());
    uLongf l1 = compressBound((uLong)v.size());
    std::vector<uint8_t> tmp(l1);
    compress2(tmp.data(), &l1, v.data(), (uLong)v.size(), 1);
    printf("%-28s n %8zu -> %8zu (zlib-1 %8lu, stored chunks %zu, unlimited depth %2d) %s crc %s\n", name.c_str(), v.size(), s.size(), (unsigned long)l1, stored,
           deepest_ll, ok ? "ok" : "FAIL", c == zc ? "ok" : "FAIL");
    if (!ok || c != zc) ++failures;
}

// order-2 de Bruijn sequence over k symbols by Lyndon words: every ordered pair occurs once among its k * k entries
static void de_bruijn2(int t, int p, int k, int* w, std::vector<uint8_t>& seq) {
    if (t > 2) {
        if (2 % p == 0) for (int i = 1; i <= p; ++i) seq.push_back((uint8_t)w[i]);
        return;
    }
    w[t] = w[t - p];
    de_bruijn2(t + 1, p, k, w, seq);
    for (int j = w[t - p] + 1; j < k; ++j) { w[t] = j; de_bruijn2(t + 1, t, k, w, seq); }
}

// the length limiter alone: Fibonacci weights need n - 1 bits without it; the limited code must be complete (Kraft sum exactly 1)
static void check_limit(int n, int maxbits) {
    std::vector<Small> small(1);
    std::vector<uint32_t> freq(288, 0);
    std::vector<uint8_t> lens(288, 0xFF);
    uint32_t a = 1, b = 1;
    for (int i = 0; i < n; ++i) { freq[7 * i % n] = a;   /* 7 is coprime to every n used: a permutation */ const uint32_t c = a + b; a = b; b = c; }
    const int depth = huffman_depth(freq.data(), n);
    HostX x;
    build_lengths(x, small[0], freq.data(), n, maxbits, lens.data());
    uint64_t kraft = 0;
    int longest = 0;
    for (int i = 0; i < n; ++i) { kraft += 1ull << (maxbits - lens[i]); longest = std::max<int>(longest, lens[i]); }
    const bool ok = depth == n - 1 && longest == maxbits && kraft == (1ull << maxbits);
    printf("limit %2d bits on %2d Fibonacci weights: unlimited depth %2d, longest %2d, Kraft %s %s\n", maxbits, n, depth, longest,
           kraft == (1ull << maxbits) ? "complete" : "BROKEN", ok ? "ok" : "FAIL");
    if (!ok) ++failures;
}

int main(int argc, char** argv) {
    std::mt19937 rng(7);
    check_limit(22, 15); check_limit(30, 15); check_limit(12, 7); check_limit(19, 7);
    const int lens[] = {1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 262, 1023, 1024, 1025, CH - 1, CH, CH + 1, CH + 2, 2 * CH + 7, 5 * CH + 1};
    check("empty", {});
    for (int n : lens) {
        std::vector<uint8_t> v(n, 0);
        check("zeros", v);
        for (auto& b : v) b = (uint8_t)rng();
        check("random", v);
        const uint8_t sym[4] = {'a', 'c', 'g', 't'};
        for (auto& b : v) { const unsigned r = rng() % 100; b = sym[r < 70 ? 0 : r < 90 ? 1 : r < 98 ? 2 : 3]; }
        check("skewed4", v);
        for (int i = 0; i < n; ++i) v[i] = (uint8_t)(i % 251);
        check("mod251", v);
        for (int i = 0; i < n; ++i) v[i] = (uint8_t)((i & 1) ? 0x55 : 0xAA);
        check("alternating", v);
    }
    for (int period : {1, 2, 3, 4, 8, 224, 896, CH - 1}) {
        std::vector<uint8_t> base(period), v(3 * CH + 5);
        for (auto& b : base) b = (uint8_t)rng();
        for (size_t i = 0; i < v.size(); ++i) v[i] = base[i % period];
        check("period " + std::to_string(period), v);
    }
    {   // Fibonacci counts: an unrestricted Huffman tree is 20 deep, the 15-bit limit acts
        std::vector<uint8_t> v;
        unsigned a = 1, b = 1;
        for (int s = 0; s < 21; ++s) { v.insert(v.end(), a, (uint8_t)(40 + s)); const unsigned c = a + b; a = b; b = c; }
        std::shuffle(v.begin(), v.end(), rng);
        check("fibonacci 21", v);
    }
    {   // a chunk in which the 15-bit limit acts: 18 symbols with counts 1, 2, 3, 5, ... 4181 on the even bytes, 128 others on the odd bytes in
        // de Bruijn order (every ordered pair once), so no 4-byte string repeats, nothing matches and the coder sees the byte counts
        std::vector<uint8_t> steep, pairs;
        unsigned a = 1, b = 2;
        for (int s = 0; s < 18; ++s) { steep.insert(steep.end(), a, (uint8_t)(3 + 5 * s)); const unsigned c = a + b; a = b; b = c; }
        std::shuffle(steep.begin(), steep.end(), rng);
        int w[4] = {0, 0, 0, 0};
        de_bruijn2(1, 1, 128, w, pairs);
        std::vector<uint8_t> v(2 * steep.size());
        for (size_t i = 0; i < steep.size(); ++i) { v[2 * i] = steep[i]; v[2 * i + 1] = (uint8_t)(128 + pairs[i]); }
        check("steep literal-only chunk", v);
        if (deepest_ll <= 15) { printf("FAIL: the steep chunk's unrestricted tree is only %d deep\n", deepest_ll); ++failures; }
    }
    {   // a float32 image and a label volume, as the folders hold them
        const int Z = 4, Y = 128, X = 112;
        std::vector<float> img(Z * Y * X), lab(Z * Y * X);
        std::normal_distribution<float> nd(0.f, 0.1f);
        for (int z = 0; z < Z; ++z)
            for (int y = 0; y < Y; ++y)
                for (int x = 0; x < X; ++x) {
                    const bool zero = y < Y / 6 || x < X / 7;
                    img[(z * Y + y) * X + x] = zero ? 0.f : sinf(y / 17.f) + cosf(x / 23.f) + nd(rng);
                    const float r = hypotf(y - Y / 2.f, x - X / 2.f);
                    lab[(z * Y + y) * X + x] = r < 10 ? 3.f : r < 20 ? 2.f : r < 35 ? 1.f : 0.f;
                }
        std::vector<uint8_t> v(img.size() * 4);
        memcpy(v.data(), img.data(), v.size());
        check("float32 image", v);
        memcpy(v.data(), lab.data(), v.size());
        check("float32 labels", v);
    }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> v;
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) v.insert(v.end(), chunk, chunk + got);
        fclose(f);
        check(argv[a], v);
        std::vector<uint8_t> s = deflate_host(v);
        s.push_back(3); s.push_back(0);
        FILE* o = fopen((std::string(argv[a]) + ".deflate").c_str(), "wb");
        if (o) { fwrite(s.data(), 1, s.size(), o); fclose(o); }
    }
    printf(failures ? "%d FAILURES\n" : "all streams inflate to their sources, all CRCs equal zlib's\n", failures);
    return failures ? 1 : 0;
}
