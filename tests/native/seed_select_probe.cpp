// Stand-alone driver of csrc/seed_select.h's host path (tests/test_seed_device.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it as a program).
//   seed_select_probe file <lum.f32> <weights.f32 | -> <seed> <stream> <n_select>   one JSON line: rc, mean, total (hex floats), picks
//   seed_select_probe sizes                                                         n = 1, 255, 256, 257 on generated samples
// Every result is also checked here against a plain restatement of the rule that shares no loop with the header: the blocked
// inclusive prefix written out as one array, the pick by std::lower_bound over it, the ordering by std::sort.
#include "seed_select.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<float> read_f32(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<float> v((size_t) bytes / sizeof(float));
    if (fread(v.data(), sizeof(float), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return v;
}

// the rule once more, the slow way
static int plain(const std::vector<float> &lum, const float *wts, uint64_t seed, uint32_t stream, uint32_t n_select, std::vector<uint32_t> &picks, double &mean,
                 double &total) {
    const size_t n = lum.size();
    std::vector<double> incl(n), boff;
    double off = 0.0, sum = 0.0, tok = 0.0;
    for (size_t lo = 0; lo < n; lo += SEED_BLOCK) {
        double w = 0.0, s = 0.0, t = 0.0;
        for (size_t i = lo; i < std::min(n, lo + SEED_BLOCK); ++i) {
            const float l = lum[i], lw = wts ? wts[i] : l;
            if (!std::isnan(l)) {
                t += 1.0;
                s += (double) l;
                if (l != 0.f && lw > 0.f && std::isfinite(lw)) w += (double) lw;
            }
            incl[i] = w;
        }
        boff.push_back(off);
        off += w; sum += s; tok += t;
    }
    for (size_t i = 0; i < n; ++i) incl[i] = boff[i / SEED_BLOCK] + incl[i];
    total = off;
    mean = tok > 0 ? sum / tok : 0.0;
    if (!(mean > 0.0)) return SEED_SELECT_ZERO_MEAN;
    if (!(total > 0.0)) return SEED_SELECT_NO_WEIGHT;
    picks.clear();
    for (uint32_t j = 0; j < n_select; ++j) {
        const float xi = (float) (seed_philox0((uint32_t) seed, (uint32_t) (seed >> 32), 0u, j, stream, SEED_TAG_SEEDSEL) >> 8) * (1.0f / 16777216.0f);
        const double target = (double) xi * total;
        size_t i = (size_t) (std::lower_bound(incl.begin(), incl.end(), target) - incl.begin());
        if (i >= n) i = n - 1;
        while (i + 1 < n && !(incl[i] > (i ? incl[i - 1] : 0.0))) ++i;            // zero width: the next entry that has one
        while (i > 0 && !(incl[i] > incl[i - 1])) --i;                            // ... or, past the end, the last one
        picks.push_back((uint32_t) i);
    }
    std::sort(picks.begin(), picks.end());
    return SEED_SELECT_OK;
}

static int run(const std::vector<float> &lum, const float *wts, uint64_t seed, uint32_t stream, uint32_t n_select, bool print) {
    std::vector<uint32_t> got(n_select, 0xffffffffu), want;
    double mean = 0.0, total = 0.0, mean_p = 0.0, total_p = 0.0;
    const int rc = seed_select_host(lum.data(), wts, (uint32_t) lum.size(), (uint32_t) seed, (uint32_t) (seed >> 32), stream, n_select, 1.0, got.data(), &mean, &total);
    const int rc_p = plain(lum, wts, seed, stream, n_select, want, mean_p, total_p);
    if (rc != rc_p || memcmp(&mean, &mean_p, sizeof mean) || memcmp(&total, &total_p, sizeof total)) {
        fprintf(stderr, "n = %zu: status / mean / total differ from the plain restatement: %d %a %a against %d %a %a\n", lum.size(), rc, mean, total, rc_p, mean_p, total_p);
        return 1;
    }
    if (rc == SEED_SELECT_OK) {
        for (uint32_t j = 0; j < n_select; ++j) {
            if (got[j] != want[j]) { fprintf(stderr, "n = %zu: pick %u is sample %u, the plain restatement has %u\n", lum.size(), j, got[j], want[j]); return 1; }
            if (!(seed_weight(lum[got[j]], wts ? wts[got[j]] : lum[got[j]]) > 0.0)) { fprintf(stderr, "n = %zu: pick %u (sample %u) has no weight\n", lum.size(), j, got[j]); return 1; }
        }
    }
    if (print) {
        printf("{\"rc\": %d, \"mean\": \"%a\", \"total\": \"%a\", \"picks\": [", rc, mean, total);
        for (uint32_t j = 0; rc == SEED_SELECT_OK && j < n_select; ++j) printf("%s%u", j ? ", " : "", got[j]);
        printf("]}\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "file")) {
        const std::vector<float> lum = read_f32(argv[2]);
        std::vector<float> wts;
        if (strcmp(argv[3], "-")) wts = read_f32(argv[3]);
        if (lum.empty() || (!wts.empty() && wts.size() != lum.size())) { fprintf(stderr, "empty samples, or weights of another length\n"); return 2; }
        return run(lum, wts.empty() ? nullptr : wts.data(), strtoull(argv[4], nullptr, 0), (uint32_t) strtoul(argv[5], nullptr, 0), (uint32_t) strtoul(argv[6], nullptr, 0), true);
    }
    if (argc == 2 && !strcmp(argv[1], "sizes")) {
        for (uint32_t n : {1u, 255u, 256u, 257u}) {
            std::vector<float> lum(n), wts(n);
            uint32_t s = 12345u + n;
            for (uint32_t i = 0; i < n; ++i) {
                s = s * 1664525u + 1013904223u;
                lum[i] = (s >> 28) == 0 ? 0.f : std::ldexp((float) (s >> 8), -20 - (int) ((s >> 4) & 15u)); // zeros and four decades
                s = s * 1664525u + 1013904223u;
                wts[i] = (s >> 29) == 0 ? 0.f : (float) (s >> 8) * (1.0f / 16777216.0f);
            }
            if (n > 1) lum[n / 2] = std::nanf("");
            if (n == 1) lum[0] = 0.75f, wts[0] = 2.f;
            for (uint32_t stream : {0u, 3u}) {
                if (run(lum, nullptr, 0x5EEDull, stream, 97, false)) return 1;
                if (run(lum, wts.data(), 12345678901234ull, stream, 97, false)) return 1;
            }
        }
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: seed_select_probe file <lum.f32> <weights.f32 | -> <seed> <stream> <n_select> | seed_select_probe sizes\n");
    return 2;
}
