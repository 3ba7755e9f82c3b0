// tt_plan_main.cpp -- the planner of the tensor-train handle (csrc/tt_plan.h, csrc/pcx_tt_plan.hip) as a stand-alone
// program, for tests/test_tt_plan_host.py: built with the address and undefined-behaviour sanitizers on the host side.
// No HIP call is made: the program needs no GPU.  It is also how a plan is printed on any machine:
//
//   echo "5 5  11 11 11 11 11  1 8 8 8 6 1  0 1 2 3 4  42 0" | tt_plan_main
//
// Input (a file named on the command line, else stdin), one model per line:
//   d len  n_0 .. n_{len-1}  r_0 .. r_len  o_0 .. o_{len-1}  seed  bad
// d is what tt_make_plan is told, len the length of the arrays it is given (the same but for a d out of range); o is
// dim_order.  The domain of dimension k is [-1 - k/8, 1 + k/4].  bad: 0 a sound model, 1 .. 4 n_nodes / ranks / lo / hi
// missing, 5 no dim_order (NULL: storage order = user order), 10 + k: lo = hi in dimension k.  The cores are exactly
// core_total doubles, core[i] = splitmix64(seed + i + 1) / 2^64 - 1/2 (tests/tt_plan_rule.py: cores()).
// Output, one JSON object per model: "rc" and "error" of tt_make_plan; every field of TTPlan ("plan"); the five LDS sizes
// ("lds"); tt_auto_variant for the requested variants 0 .. 4 with every image uploaded ("auto_all") and with the
// lane-per-point image missing ("auto_nolpp"), a refusal as its message; the host-built tables ("tables"): entries in full
// up to 2,000 of them, else length and SHA-256 of their bytes.
#include "pcx_internal.h"
#include "tt_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

PCX_HIDDEN char *pcx_err_buf() noexcept {         // the library keeps it in pcx_core.hip
    static thread_local char buf[PCX_ERR_LEN];
    return buf;
}

// SHA-256 (FIPS 180-4) of a byte string, as 64 hex digits
static void sha256_hex(const unsigned char *msg, size_t len, char hex[65]) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<unsigned char> m(msg, msg + len);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; --i) m.push_back((unsigned char)(((uint64_t)len * 8) >> (8 * i)));
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t blk = 0; blk < m.size(); blk += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)m[blk + 4 * i] << 24 | (uint32_t)m[blk + 4 * i + 1] << 16 | (uint32_t)m[blk + 4 * i + 2] << 8 | m[blk + 4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    for (int i = 0; i < 8; ++i) snprintf(hex + 8 * i, 9, "%08x", h[i]);
}

static const size_t kFullTable = 2000;

static void put_table(const char *name, const std::vector<double> &v, bool &first) {
    printf("%s\"%s\": {\"len\": %zu", first ? "" : ", ", name, v.size());
    first = false;
    if (v.size() <= kFullTable) {
        printf(", \"data\": [");
        for (size_t i = 0; i < v.size(); ++i) printf("%s%.17g", i ? "," : "", v[i]);
        printf("]}");
        return;
    }
    char hex[65];
    sha256_hex((const unsigned char *)v.data(), v.size() * sizeof(double), hex);
    printf(", \"sha256\": \"%s\"}", hex);
}

template <typename T>
static void put_ints(const char *name, const T *v, int count) {
    printf(", \"%s\": [", name);
    for (int i = 0; i < count; ++i) printf("%s%ld", i ? ", " : "", (long)v[i]);
    printf("]");
}

static void put_doubles(const char *name, const double *v, int count) {
    printf(", \"%s\": [", name);
    for (int i = 0; i < count; ++i) printf("%s%.17g", i ? ", " : "", v[i]);
    printf("]");
}

static void put_plan(const TTPlan &p) {
    const int d = p.dims.d;
#define F(x) printf(", \"" #x "\": %ld", (long)p.x)
    printf(", \"plan\": {\"d\": %d", d);
    put_ints("n", p.dims.n, d); put_ints("col", p.dims.col, d); put_doubles("lo", p.dims.lo, d); put_doubles("hi", p.dims.hi, d);
    put_doubles("scale", p.dims.scale, d); put_ints("frag_off", p.dims.frag_off, d);
    put_ints("ranks", p.ranks, d + 1); put_ints("coff", p.coff, d);
    F(core_total); F(frag_total); F(rmax); F(nmax); F(generic);
    put_ints("gi.rank", p.gi.rank, d + 1); put_ints("gi.coff", p.gi.coff, d); F(gi.rmax); F(gi.nmax);
    F(cls); put_ints("rk.rc", p.rk.rc, d); put_ints("rk.rt", p.rk.rt, d); F(rl_last); F(last_rows); F(last_lds_doubles);
    F(wR); put_ints("wplan.ntiles", p.wplan.ntiles, d); put_ints("wplan.lds_off", p.wplan.lds_off, d); F(wplan.ks); F(wplan.total);
    F(d4RA); put_ints("d4plan.lds_off", p.d4plan.lds_off, d); F(d4plan.total); F(d4_preferred);
    F(lppCap); F(lpp_nodes); F(lpp_preferred);
#undef F
    printf("}");
}

static void put_auto(const char *name, const TTPlan &p, const TTImages &up) {
    printf(", \"%s\": [", name);
    for (int v = 0; v <= 4; ++v) {
        const int form = tt_auto_variant(p, up, v);
        if (form >= 0) printf("%s%d", v ? ", " : "", form);
        else printf("%s\"%s\"", v ? ", " : "", pcx_err_buf());
        if ((form >= 0) != tt_plan_has_variant(p, up, v)) { fprintf(stderr, "tt_plan_main: tt_plan_has_variant disagrees\n"); exit(3); }
    }
    printf("]");
}

static uint64_t splitmix64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

int main(int argc, char **argv) {
    FILE *in = stdin;
    if (argc > 1 && !(in = fopen(argv[1], "r"))) { fprintf(stderr, "tt_plan_main: cannot open %s\n", argv[1]); return 2; }
    int d, len;
    while (fscanf(in, "%d %d", &d, &len) == 2) {
        if (len < 1 || len > 64) { fprintf(stderr, "tt_plan_main: len=%d\n", len); return 2; }
        std::vector<int32_t> n((size_t)len), ranks((size_t)len + 1), order((size_t)len);      // exact sizes: a read past them is the sanitizer's
        long seed, bad;
        bool ok = true;
        for (int32_t &v : n) ok = ok && fscanf(in, "%d", &v) == 1;
        for (int32_t &v : ranks) ok = ok && fscanf(in, "%d", &v) == 1;
        for (int32_t &v : order) ok = ok && fscanf(in, "%d", &v) == 1;
        if (!ok || fscanf(in, "%ld %ld", &seed, &bad) != 2) { fprintf(stderr, "tt_plan_main: short line\n"); return 2; }
        std::vector<double> lo((size_t)len), hi((size_t)len);
        for (int k = 0; k < len; ++k) { lo[k] = -1.0 - 0.125 * k; hi[k] = 1.0 + 0.25 * k; }
        if (bad >= 10 && bad - 10 < len) hi[bad - 10] = lo[bad - 10];

        TTPlan p;
        const int rc = tt_make_plan(d, bad == 1 ? nullptr : n.data(), bad == 2 ? nullptr : ranks.data(), bad == 3 ? nullptr : lo.data(),
                                    bad == 4 ? nullptr : hi.data(), bad == 5 ? nullptr : order.data(), p);
        printf("{\"rc\": %d", rc);
        if (rc != PCX_OK) {
            printf(", \"error\": \"%s\"}\n", pcx_err_buf());
            continue;
        }
        put_plan(p);
        printf(", \"lds\": {\"generic\": %zu, \"d4\": %zu, \"wfirst\": [%zu, %zu], \"direct\": [%zu, %zu, %zu], \"lpp\": %zu}",
               tt_generic_lds_bytes(p), tt_d4_lds_bytes(p), tt_wfirst_lds_bytes(p, 1), tt_wfirst_lds_bytes(p, 4),
               tt_direct_lds_bytes(p, 1), tt_direct_lds_bytes(p, 2), tt_direct_lds_bytes(p, 4), tt_lpp_lds_bytes(p));
        put_auto("auto_all", p, TTImages{true, true, true});
        put_auto("auto_nolpp", p, TTImages{true, true, false});

        std::vector<double> cores((size_t)p.core_total);
        for (size_t i = 0; i < cores.size(); ++i)
            cores[i] = (double)(splitmix64((uint64_t)seed + i + 1) >> 11) * 0x1p-53 - 0.5;
        printf(", \"tables\": {");
        bool first = true;
        if (!p.generic) put_table("last", tt_pack_last_core(p, cores.data()), first);
        if (p.d4RA) put_table("d4", tt_pack_d4_image(p, cores.data()), first);
        if (p.lppCap) {
            put_table("lpp", tt_pack_lpp_image(p, cores.data()), first);
            printf(", \"lpp_tab\": [");
            const std::vector<TTLppDim> tab = tt_lpp_table(p);
            for (size_t k = 0; k < tab.size(); ++k)
                printf("%s[%d, %d, %d, %d, %d, %d, %.17g, %.17g]", k ? ", " : "", tab[k].off, tab[k].rl, tab[k].rr, tab[k].n, tab[k].col,
                       tab[k].pad_, tab[k].lo, tab[k].scale);
            printf("]");
        }
        printf("}}\n");
    }
    return 0;
}
