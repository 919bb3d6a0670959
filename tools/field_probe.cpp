// How many field lookups ("jumps") does a lidar beam need?  Host-only experiment behind the choice of the free-space
// field of the ray cast (csrc/mrca_host.h): the march is exact for ANY field of valid empty rectangles, so the field
// only decides the jump count -- which the kernel's VALU-bound half is proportional to.
//
//   (a) the round-1..3 field: ONE rectangle per cell, grown greedily on all four sides (a ray only ever uses the two
//       extents that face its direction of travel; the growth of the other two sides narrows them) -- 1.7 lookups per beam
//       on the Stage-1 rink; the product no longer builds it, the figure is in DESIGN.md 5.2;
//   (b) QUADRANT fields: four rectangles per cell, each with the cell in the corner the ray ENTERS through (a ray of
//       quadrant (+,+) looks up the rectangle that extends right and up only), grown greedily on its two sides: counted
//       with a float walk of this file's own (policies: alternate growth, largest area, squares);
//   (c) OCTANT fields (mrca_host.h: build_octant_rect_field): eight per cell, each quadrant's rectangle grown with a bias
//       toward the ray's major axis -- counted by the product's own march (grid_march_skip over a field that counts its
//       lookups), trips as the kernel's loop takes them, a wave = 64 consecutive beams: growth 2 : 1, 3 : 2 and 3 : 1, extents
//       capped at 121 cells, for every jump or for every jump after the first (the origin's jump keeps the quadrant entry a
//       `head` record carries: the form the product runs).
//
//   python tools/field_probe.py          # writes the three shipped maps, builds this file, runs it on each
//   g++ -O2 -std=c++17 -pthread tools/field_probe.cpp -o tools/_build/field_probe && tools/_build/field_probe map.bin [robots] [half]
// map.bin = int32 width, height, wpr; float cell, x0, y0; uint32 bits[height*wpr]   (tools/field_probe.py writes it)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../rl-collision-avoidance_amd/csrc/mrca_host.h"

using namespace mrca;

struct Map {
    int32_t w, h, wpr;
    float cell, x0, y0;
    std::vector<uint32_t> bits;
    bool occ(int x, int y) const {
        if (x < 0 || y < 0 || x >= w || y >= h) return false;
        return (bits[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u;
    }
};

// quadrant q = (sx > 0) | (sy > 0) << 1; entry = ex | ey << 8 (cells beyond the cell itself in the travel direction)
static void build_quadrant(const Map& m, int q, std::vector<uint16_t>* out, int policy) {
    const int sx = (q & 1) ? 1 : -1, sy = (q & 2) ? 1 : -1;
    const size_t sw = (size_t)m.w + 1;
    std::vector<int32_t> sat(sw * ((size_t)m.h + 1), 0);
    for (int y = 0; y < m.h; ++y)
        for (int x = 0; x < m.w; ++x)
            sat[(size_t)(y + 1) * sw + x + 1] =
                (int)m.occ(x, y) + sat[(size_t)y * sw + x + 1] + sat[(size_t)(y + 1) * sw + x] - sat[(size_t)y * sw + x];
    auto count = [&](int x0, int y0, int x1, int y1) -> int {
        if (x0 > x1) std::swap(x0, x1);
        if (y0 > y1) std::swap(y0, y1);
        x0 = std::max(x0, 0); y0 = std::max(y0, 0); x1 = std::min(x1, m.w - 1); y1 = std::min(y1, m.h - 1);
        if (x0 > x1 || y0 > y1) return 0;
        return sat[(size_t)(y1 + 1) * sw + x1 + 1] - sat[(size_t)y0 * sw + x1 + 1] - sat[(size_t)(y1 + 1) * sw + x0] +
               sat[(size_t)y0 * sw + x0];
    };
    out->assign((size_t)m.w * m.h, 0xFFFF);
    const int M = 254;
    for (int y = 0; y < m.h; ++y)
        for (int x = 0; x < m.w; ++x) {
            if (m.occ(x, y)) continue;
            int ex = 0, ey = 0;
            if (policy == 0) {          // alternate
                for (bool grew = true; grew;) {
                    grew = false;
                    if (ex < M && count(x + sx * (ex + 1), y, x + sx * (ex + 1), y + sy * ey) == 0) { ++ex; grew = true; }
                    if (ey < M && count(x, y + sy * (ey + 1), x + sx * ex, y + sy * (ey + 1)) == 0) { ++ey; grew = true; }
                }
            } else if (policy == 3) {   // the corner rectangle of the largest AREA (staircase enumeration)
                long long best = -1;
                int w = M;
                for (int h = 0; h <= M; ++h) {
                    // widest free run in row y + sy*h, limited by the rows below it
                    int run = 0;
                    if (m.occ(x, y + sy * h)) break;
                    while (run < w && !m.occ(x + sx * (run + 1), y + sy * h)) ++run;
                    w = std::min(w, run);
                    const long long area = (long long)(w + 1) * (h + 1);
                    if (area > best) { best = area; ex = w; ey = h; }
                }
            } else if (policy == 2) {   // the largest SQUARE only (one byte per quadrant)
                while (ex < M && count(x, y, x + sx * (ex + 1), y + sy * (ex + 1)) == 0) ++ex;
                ey = ex;
            } else {                    // the largest SQUARE first, then alternate
                while (ex < M && count(x, y, x + sx * (ex + 1), y + sy * (ex + 1)) == 0) ++ex;
                ey = ex;
                for (bool grew = true; grew;) {
                    grew = false;
                    if (ex < M && count(x + sx * (ex + 1), y, x + sx * (ex + 1), y + sy * ey) == 0) { ++ex; grew = true; }
                    if (ey < M && count(x, y + sy * (ey + 1), x + sx * ex, y + sy * (ey + 1)) == 0) { ++ey; grew = true; }
                }
            }
            (*out)[(size_t)y * m.w + x] = (uint16_t)(ex | (ey << 8));
        }
}

// returns the number of field lookups AFTER the origin's own entry (which every beam of a robot shares)
template <class Ext>
static int march_count(const Map& m, float ox, float oy, float dx, float dy, float tmax, Ext ext, float* range) {
    const double fx = (ox - m.x0) / m.cell, fy = (oy - m.y0) / m.cell, tmc = tmax / m.cell;
    int ix = (int)std::floor(fx), iy = (int)std::floor(fy);
    const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
    int lookups = 0;
    *range = tmax;
    if (m.occ(ix, iy)) { *range = 0; return 0; }
    for (int guard = 0; guard < 4096; ++guard) {
        int ex, ey;
        ext(ix, iy, sx, sy, &ex, &ey);
        const int Bx = sx > 0 ? ix + ex + 1 : ix - ex, By = sy > 0 ? iy + ey + 1 : iy - ey;
        const double tBx = dx != 0 ? (Bx - fx) / dx : 1e30, tBy = dy != 0 ? (By - fy) / dy : 1e30;
        const bool xe = tBx < tBy;
        const double t = xe ? tBx : tBy;
        if (t >= tmc) return lookups;
        const double px = fx + dx * t, py = fy + dy * t;
        if (xe) { ix = sx > 0 ? Bx : Bx - 1; iy = (int)std::floor(py); }
        else    { iy = sy > 0 ? By : By - 1; ix = (int)std::floor(px); }
        ++lookups;
        if (m.occ(ix, iy)) { *range = (float)(t * m.cell); return lookups; }
    }
    return lookups;
}

// a field that counts its lookups and remembers the last entry it returned
struct Counting {
    FreeRectField f;
    mutable int lookups = 0;
    mutable uint32_t last = 0;
    uint32_t entry_bytes(float dx, float dy) const { return f.entry_bytes(dx, dy); }
    uint32_t operator()(int ix, int iy, uint32_t qb) const { ++lookups; return last = f(ix, iy, qb); }
};

// (c): `robots` seeded poses uniform in the free cells of the +-half square, 512 beams each, the product's march.
// origin_octant: the origin's jump takes the octant entry too (a `head` record of 32 bytes would carry it)
static void octant_row(const Map& m, const GridGeom& g, const char* label, const FreeRectField& quad, const FreeRectField& later,
                       bool origin_octant, int robots, float half) {
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    long long looks = 0, trips = 0, waves = 0, beams = 0, hist[12] = {0};
    for (int r = 0; r < robots; ++r) {
        float x, y;
        do {
            x = U(rng) * half;
            y = U(rng) * half;
        } while (m.occ((int)std::floor((x - m.x0) / m.cell), (int)std::floor((y - m.y0) / m.cell)));
        const float th = U(rng) * 3.14159265f;
        const MarchOrigin org0 = march_origin(quad, g, x, y);
        int wmax = 0;
        for (int b = 0; b < 512; ++b) {
            const double a = th - M_PI / 2 + b * M_PI / 511;
            const float dx = (float)std::cos(a), dy = (float)std::sin(a);
            MarchOrigin org = org0;
            if (origin_octant) {
                const uint32_t e = later(org.ix0, org.iy0, later.entry_bytes(dx, dy));
                org.v_lo = org.v_hi = e | e << 16;
            }
            Counting cf{later};
            const uint32_t vq = dy > 0.0f ? org.v_hi : org.v_lo;
            cf.last = dx > 0.0f ? vq >> 16 : vq & 0xFFFFu;
            (void)grid_march_skip(cf, g, org, dx, dy, 6.0f);
            // a trip looks up once unless it is the one that finds the beam's end (t >= tmax); a hit ends in a lookup
            const int t = cf.lookups + (cf.last == kCellOccupied ? 0 : 1);
            looks += cf.lookups;
            ++hist[std::min(t, 11)];
            wmax = std::max(wmax, t);
            ++beams;
            if ((b & 63) == 63) { trips += wmax; ++waves; wmax = 0; }
        }
    }
    printf("  %-58s %.3f lookups / beam  %.3f trips / wave   trips per beam:", label, (double)looks / beams, (double)trips / waves);
    for (int k = 1; k < 10; ++k) printf(" %d:%.3f", k, (double)hist[k] / beams);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    Map m;
    if (fread(&m.w, 4, 1, f) != 1 || fread(&m.h, 4, 1, f) != 1 || fread(&m.wpr, 4, 1, f) != 1 || fread(&m.cell, 4, 1, f) != 1 ||
        fread(&m.x0, 4, 1, f) != 1 || fread(&m.y0, 4, 1, f) != 1)
        return 1;
    m.bits.resize((size_t)m.h * m.wpr);
    if (fread(m.bits.data(), 4, m.bits.size(), f) != m.bits.size()) return 1;
    fclose(f);
    const int robots = argc > 2 ? atoi(argv[2]) : 2000;
    const float rmax = argc > 3 ? (float)atof(argv[3]) : 9.0f;        // robots uniform in a disc of this radius (stage 1)
    std::vector<uint16_t> field;
    int pitch = 0;
    build_free_rect_field(m.bits.data(), m.w, m.h, m.wpr, &field, &pitch);
    std::vector<uint16_t> quad[4][4];
    for (int pol = 0; pol < 4; ++pol)
        for (int q = 0; q < 4; ++q) build_quadrant(m, q, &quad[pol][q], pol);
    auto make_q = [&](int pol) {
        return [&, pol](int ix, int iy, int sx, int sy, int* ex, int* ey) {
            if (ix < 0 || iy < 0 || ix >= m.w || iy >= m.h) { *ex = *ey = 0; return; }
            const uint16_t v = quad[pol][(sx > 0) | ((sy > 0) << 1)][(size_t)iy * m.w + ix];
            *ex = v & 255;
            *ey = v >> 8;
        };
    };
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    long long lq[3] = {0, 0, 0}, beams = 0, mism = 0; long long wave_s = 0; int wmax_s = 0;
    long long hist_q[16] = {0};
    long long wave_q = 0, waves = 0;      // per 64-beam wavefront: the MAXIMUM over its lanes is what it executes
    for (int r = 0; r < robots; ++r) {
        float x, y;
        do {
            x = U(rng) * rmax;
            y = U(rng) * rmax;
        } while (x * x + y * y > rmax * rmax ||
                 m.occ((int)std::floor((x - m.x0) / m.cell), (int)std::floor((y - m.y0) / m.cell)));
        const float th = U(rng) * 3.14159265f;
        int wmax_q = 0;
        for (int b = 0; b < 512; ++b) {
            const double a = th - 3.14159265358979 / 2 + b * 3.14159265358979 / 511;
            const float dx = (float)std::cos(a), dy = (float)std::sin(a);
            float rq;
            const int cq0 = march_count(m, x, y, dx, dy, 6.0f, make_q(0), &rq);
            const int cq1 = march_count(m, x, y, dx, dy, 6.0f, make_q(3), &rq);
            float rs;
            const int cq2 = march_count(m, x, y, dx, dy, 6.0f, make_q(2), &rs);
            lq[0] += cq0; lq[1] += cq1; lq[2] += cq2;
            wmax_s = std::max(wmax_s, cq2 + (rs >= 6.0f ? 1 : 0));
            if ((b & 63) == 63) { wave_s += wmax_s; wmax_s = 0; }
            ++beams;
            mism += std::fabs(rs - rq) > 1e-4f;
            ++hist_q[std::min(cq0, 15)];
            // loop iterations = lookups + 1 unless the beam ended in a hit (the last iteration then found the wall)
            const int iq = cq0 + (rq >= 6.0f ? 1 : 0);
            wmax_q = std::max(wmax_q, iq);
            if ((b & 63) == 63) {
                wave_q += wmax_q; ++waves;
                wmax_q = 0;
            }
        }
    }
    printf("map %d x %d cells of %.3f m, %d robots x 512 beams\n", m.w, m.h, m.cell, robots);
    printf("lookups per beam after the origin's own entry (jumps = lookups + 1 when the beam ends beyond the last rectangle):\n");
    printf("  quadrant corner rectangles, alternate growth  %.3f\n", (double)lq[0] / beams);
    printf("  quadrant corner rectangles, LARGEST AREA      %.3f\n", (double)lq[1] / beams);
    printf("  quadrant corner SQUARES (one byte per quadrant) %.3f lookups, wavefront iterations %.3f\n", (double)lq[2] / beams,
           (double)wave_s / waves);
    printf("  loop iterations a 64-beam WAVEFRONT executes per beam pass (max over its lanes): quadrant, alternate growth %.3f\n",
           (double)wave_q / waves);
    printf("  range mismatches between fields (float walk, diagnostics only): %lld of %lld\n", mism, beams);
    printf("  histogram of lookups  quadrant: ");
    for (int k = 0; k < 10; ++k) printf("%d:%.3f ", k, (double)hist_q[k] / beams);
    printf("\n");
    // (c) the product's march over the product's builders
    GridGeom g;
    g.x0 = m.x0; g.y0 = m.y0; g.cell = m.cell; g.inv_cell = 1.0f / m.cell;
    g.width = m.w; g.height = m.h; g.wpr = m.wpr;
    const FreeRectField quad_f{field.data(), m.w, m.h, pitch};
    printf("the product's march (grid_march_skip), trips as the kernel's loop takes them, waves of 64 consecutive beams:\n");
    octant_row(m, g, "quadrant array for every lookup (MRCA_FIELD_OCTANTS=0)", quad_f, quad_f, false, robots, rmax);
    const struct { int rx, ry, cap; const char* name; } pol[] = {{2, 1, 254, "2 : 1"}, {3, 2, 254, "3 : 2"}, {3, 1, 254, "3 : 1"},
                                                                 {2, 1, 121, "2 : 1, extents <= 121"}, {1, 1, 254, "1 : 1 (major axis first)"}};
    for (const auto& p : pol) {
        std::vector<uint16_t> oct;
        int p2 = 0;
        build_octant_rect_field(m.bits.data(), m.w, m.h, m.wpr, &oct, &p2, p.rx, p.ry, p.cap);
        const FreeRectField oct_f{oct.data(), m.w, m.h, p2, 4u, 8u};
        char label[128];
        snprintf(label, sizeof label, "octants %s, every jump", p.name);
        octant_row(m, g, label, quad_f, oct_f, true, robots, rmax);
        snprintf(label, sizeof label, "octants %s, the origin keeps the quadrant entry", p.name);
        octant_row(m, g, label, quad_f, oct_f, false, robots, rmax);
    }
    return 0;
}
