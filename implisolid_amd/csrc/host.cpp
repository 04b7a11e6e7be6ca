// host.cpp -- mc-settings parser, MP5-JSON -> node-program compiler, float LU inverse.
#include "host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace impli {

// ---------------------------------------------------------------------------------------------
// basic_functions.hpp:77-128.  ublas lu_factorize: per column the first row with the largest |a|
// is the pivot (index_norm_inf), the sub-column is scaled by value_type(1)/pivot, the trailing
// block gets m(r,c) -= l(r)*u(c); lu_substitute: row swaps, unit-lower forward solve, upper back
// solve with "t = e(n,l) /= u(n,n); if (t != 0) e(m,l) -= u(m,n)*t" (triangular.hpp).
bool invert_matrix12(const float in[12], float out[12]) {
    float a[4][4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) a[r][c] = in[r * 4 + c];
    a[3][0] = a[3][1] = a[3][2] = 0.f;
    a[3][3] = 1.f;
    int perm[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i) {
        int piv = i;
        float best = 0.f;
        for (int r = i; r < 4; ++r) {
            float u = std::fabs(a[r][i]);
            if (u > best) { best = u; piv = r; }
        }
        if (a[piv][i] == 0.f) return false;   // singular: the reference returns false, matrix untouched
        if (piv != i) {
            perm[i] = piv;
            for (int c = 0; c < 4; ++c) std::swap(a[piv][c], a[i][c]);
        }
        const float inv = 1.f / a[i][i];
        for (int r = i + 1; r < 4; ++r) a[r][i] *= inv;
        for (int r = i + 1; r < 4; ++r)
            for (int c = i + 1; c < 4; ++c) {
                const float p = a[r][i] * a[i][c];
                a[r][c] -= p;
            }
    }
    float e[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) e[r][c] = (r == c) ? 1.f : 0.f;
    for (int i = 0; i < 4; ++i)
        if (perm[i] != i)
            for (int c = 0; c < 4; ++c) std::swap(e[i][c], e[perm[i]][c]);
    for (int n = 0; n < 4; ++n)
        for (int l = 0; l < 4; ++l) {
            const float t = e[n][l];
            if (t != 0.f)
                for (int m = n + 1; m < 4; ++m) {
                    const float p = a[m][n] * t;
                    e[m][l] -= p;
                }
        }
    for (int n = 3; n >= 0; --n)
        for (int l = 3; l >= 0; --l) {
            const float t = (e[n][l] /= a[n][n]);
            if (t != 0.f)
                for (int m = n - 1; m >= 0; --m) {
                    const float p = a[m][n] * t;
                    e[m][l] -= p;
                }
        }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) out[r * 4 + c] = e[r][c];
    return true;
}

// ---------------------------------------------------------------------------------------------
MCSettings parse_mc_settings(const char* text) {
    Json d;
    try {
        d = Json::parse(text);
    } catch (const JsonError& e) {
        throw InputError(e.what());
    }
    MCSettings s;
    std::string why;
    float box[6];
    const char* keys[6] = {"box.xmin", "box.xmax", "box.ymin", "box.ymax", "box.zmin", "box.zmax"};
    bool ok = true;
    for (int i = 0; i < 6; ++i) {
        float v;
        if (!d.get_float(keys[i], &v) || std::isnan(v)) ok = false;
        box[i] = v;
    }
    if (!ok) {   // :176-191
        for (int i = 0; i < 6; ++i) box[i] = (i % 2) ? 1.f : -1.f;
        why += "  err2 (missing or incorrect box)";
    }
    std::memcpy(s.box, box, sizeof box);
    {   // :193-206 resolution must be an integer-valued number
        const float r = d.get_float("resolution", -1.f);
        // a value no int holds (or NaN) is not an integer resolution: converting it would be
        // undefined behaviour (the reference's cast is; found by the host sanitizer run)
        const bool fits = r > -2147483648.f && r < 2147483648.f;
        int ri = fits ? (int)r : 0;
        if (ri == -1) ri = 28;
        if (!fits || (float)ri != r) why += "  err3 (resolution must be integer)";
        s.resolution = ri;
        if (s.resolution <= 2) why += "  err4 (resolution must be > 2)";
    }
    s.vresampl_c = d.get_float("vresampl.c", 1.0f);
    s.vresampl_iters = d.get_int("vresampl.iters", 0);
    auto read_bool = [&](const char* name, bool dflt, const char* forbidden) {   // :107-141
        int v = d.get_int(name, -1);
        bool r = (v == -1) ? dflt : (v != 0);
        if (d.get_int(forbidden, 9123456) != 9123456) why += std::string("  use ") + name;
        return r;
    };
    s.projection = read_bool("projection.enabled", false, "projection.enable");
    s.qem = read_bool("qem.enabled", false, "qem.enable");
    s.subdiv = read_bool("subdiv.enabled", true, "subdiv.enable");
    s.post_subdiv_noise = d.get_float("debug.post_subdiv_noise", 0.01f);
    s.overall_repeats = d.get_int("overall_repeats", 1);
    {   // additive key, read as the reference reads its ints (true / false are no ints: the default)
        const int v = d.get_int("normals.enabled", -1);
        s.normals = v != -1 && v != 0;
    }
    {   // additive key, ints like "normals.enabled"
        const int v = d.get_int("fit_box.enabled", -1);
        s.fit_box = v != -1 && v != 0;
        int dflt = kBoundsMinDepth;   // ceil(log2(resolution)), clamped
        while (dflt < kBoundsMaxDepth && (1 << dflt) < s.resolution) ++dflt;
        s.fit_depth = d.get_int("fit_box.depth", dflt);
        s.fit_margin = d.get_int("fit_box.margin", 2);
        if (s.fit_box) {
            if (s.fit_depth < kBoundsMinDepth || s.fit_depth > kBoundsMaxDepth) why += "  fit_box.depth must be in [3, 10]";
            if (s.fit_margin < 0 || (int64_t)s.resolution - 2 * (int64_t)s.fit_margin < 1)
                why += "  fit_box.margin must leave resolution - 2 margin >= 1";
        }
    }
    s.ignore_root_matrix = d.get_bool("ignore_root_matrix", false);
    if (s.qem && !s.projection) why += "  err7 (qem needs projection)";
    if (s.resolution > 65535) why += "  resolution exceeds the reference's dim_t";
    if (!why.empty()) throw InputError("Aborting because of a problem in mc_settings_from_json. Abort reasons: " + why);
    return s;
}

// ---------------------------------------------------------------------------------------------
void bounds_edges(const float search[6], int depth, float* edges) {
    if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw InputError("bounds: depth must be in [3, 10]");
    const int N = 1 << depth;
    for (int a = 0; a < 3; ++a) {
        const float lo = search[2 * a], hi = search[2 * a + 1];
        const float width = hi - lo;
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(width))
            throw InputError("bounds: the search box must be finite with min < max on every axis");
        const float step = width / (float)N;
        float* e = edges + (size_t)a * (N + 1);
        for (int k = 0; k < N; ++k) {
            const float off = (float)k * step;   // rounded on its own (-ffp-contract=off)
            e[k] = lo + off;
        }
        e[N] = hi;
    }
}

bool fit_box(const float search[6], const float bounds[6], int resolution, int margin, float out[6]) {
    if (margin < 0 || (int64_t)resolution - 2 * (int64_t)margin < 1) return false;
    const double cells = (double)(resolution - 2 * margin), m = (double)margin;
    for (int a = 0; a < 3; ++a) {
        const double b0 = bounds[2 * a], b1 = bounds[2 * a + 1], s0 = search[2 * a], s1 = search[2 * a + 1];
        const double w = (b1 - b0) / cells;
        const double lo = std::max(s0, b0 - m * w), hi = std::min(s1, b1 + m * w);
        out[2 * a] = (float)lo;
        out[2 * a + 1] = (float)hi;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
void mass_mids(const float box[6], int depth, float* mids) {
    if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw InputError("mass: depth must be in [3, 10]");
    const int N = 1 << depth;
    std::vector<float> edges((size_t)3 * (N + 1));
    bounds_edges(box, depth, edges.data());   // validates depth and box (InputError)
    for (int a = 0; a < 3; ++a) {
        const float* e = edges.data() + (size_t)a * (N + 1);
        float* m = mids + (size_t)a * N;
        for (int k = 0; k < N; ++k) {
            const float w = e[k + 1] - e[k];
            const float half = 0.5f * w;   // rounded on its own (-ffp-contract=off)
            m[k] = e[k] + half;
            // what puts a cell's sample inside every interval box that contains the cell
            if (!(e[k] <= m[k] && m[k] <= e[k + 1])) throw InputError("mass: a cell's sample point left its cell (box too narrow for float)");
        }
    }
}

bool mass_physical(const float box[6], int depth, const uint64_t mom[10], double out[10]) {
    if (depth < kBoundsMinDepth || depth > kBoundsMaxDepth) throw InputError("mass: depth must be in [3, 10]");
    double lo[3], d[3];
    const double N = (double)(1 << depth);
    for (int a = 0; a < 3; ++a) {
        const float l = box[2 * a], h = box[2 * a + 1];
        if (!std::isfinite(l) || !std::isfinite(h) || !(l < h))
            throw InputError("mass: the box must be finite with min < max on every axis");
        lo[a] = (double)l;
        d[a] = ((double)h - (double)l) / N;
    }
    for (int k = 0; k < 10; ++k) out[k] = 0.0;
    const uint64_t n = mom[0];
    if (n == 0) return false;
    const double nd = (double)n;
    const double cell = (d[0] * d[1]) * d[2];
    const double volume = nd * cell;
    out[0] = volume;
    for (int a = 0; a < 3; ++a) out[1 + a] = lo[a] + ((double)mom[1 + a] / nd + 0.5) * d[a];
    // central second moments from exact integers: c_ab = n S_ab - S_a S_b (negative for some cross terms)
    auto mu = [&](int a, int b, uint64_t sab) {
        const __int128 c = (__int128)n * (__int128)sab - (__int128)mom[1 + a] * (__int128)mom[1 + b];
        const double q = (double)c / (nd * nd) + (a == b ? 1.0 / 12.0 : 0.0);
        return ((volume * d[a]) * d[b]) * q;
    };
    const double mxx = mu(0, 0, mom[4]), myy = mu(1, 1, mom[5]), mzz = mu(2, 2, mom[6]);
    const double mxy = mu(0, 1, mom[7]), myz = mu(1, 2, mom[8]), mxz = mu(0, 2, mom[9]);
    out[4] = myy + mzz;
    out[5] = mxx + mzz;
    out[6] = mxx + myy;
    out[7] = -mxy;
    out[8] = -myz;
    out[9] = -mxz;
    return true;
}

// ---------------------------------------------------------------------------------------------
void slice_coords(const float rect[4], int resolution, float* xs, float* ys) {
    if (resolution < 1 || resolution > kSliceMaxResolution) throw InputError("slice: resolution must be in [1, 4096]");
    for (int a = 0; a < 2; ++a) {
        const float lo = rect[2 * a], hi = rect[2 * a + 1];
        const float width = hi - lo;
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(width))
            throw InputError("slice: the rect must be finite with min < max on both axes");
        const float step = width / (float)resolution;
        float* e = a ? ys : xs;
        for (int k = 0; k < resolution; ++k) {
            const float off = (float)k * step;   // rounded on its own (-ffp-contract=off)
            e[k] = lo + off;
        }
        e[resolution] = hi;
    }
}

void raster_coords(const float rect[4], int width, int height, int supersample, float* mx, float* my) {
    if (width < 1 || width > kRasterMaxSide) throw InputError("raster: width must be in [1, 16384]");
    if (height < 1 || height > kRasterMaxSide) throw InputError("raster: height must be in [1, 16384]");
    if (supersample != 1 && supersample != 2 && supersample != 4) throw InputError("raster: supersample must be 1, 2 or 4");
    std::vector<float> edges;
    for (int a = 0; a < 2; ++a) {
        const float lo = rect[2 * a], hi = rect[2 * a + 1];
        const float width_f = hi - lo;
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(width_f))
            throw InputError("raster: the rect must be finite with min < max on both axes");
        const int n = (a ? height : width) * supersample;   // sub-cells on the axis
        const float step = width_f / (float)n;
        edges.resize((size_t)n + 1);
        for (int k = 0; k < n; ++k) {
            const float off = (float)k * step;   // rounded on its own (-ffp-contract=off)
            edges[k] = lo + off;
        }
        edges[n] = hi;
        float* m = a ? my : mx;
        for (int k = 0; k < n; ++k) {
            const float w = edges[k + 1] - edges[k];
            const float half = 0.5f * w;         // rounded on its own
            m[k] = edges[k] + half;
            // what puts a tile's samples inside the box of its first and last ones
            if (!(edges[k] <= m[k] && m[k] <= edges[k + 1]))
                throw InputError("raster: a sample point left its sub-cell (rect too narrow for float)");
        }
    }
}

void ray_params(float t0, float t1, int steps, float* ts) {
    if (steps < 1 || steps > kRayMaxSteps) throw InputError("raycast: steps must be in [1, 65536]");
    const float width = t1 - t0;
    if (!std::isfinite(t0) || !std::isfinite(t1) || !(t0 < t1) || !std::isfinite(width))
        throw InputError("raycast: the range must be finite with t0 < t1");
    const float step = width / (float)steps;
    for (int k = 0; k < steps; ++k) {
        const float off = (float)k * step;   // rounded on its own (-ffp-contract=off)
        ts[k] = t0 + off;
    }
    ts[steps] = t1;
    // what puts a segment's samples between its end samples (only ts[steps - 1] > t1 can fail)
    for (int k = 0; k < steps; ++k)
        if (!(ts[k] <= ts[k + 1])) throw InputError("raycast: the sample parameters are not non-decreasing (range too narrow for float)");
}

int64_t slice_loops(const uint32_t* keys, int64_t n, int64_t* order, int64_t* loop_offsets, uint8_t* closed) {
    loop_offsets[0] = 0;
    if (n <= 0) return 0;
    // segments sorted by start key and by end key: a repeated key among either is refused
    std::vector<std::pair<uint32_t, int64_t>> by_start((size_t)n), by_end((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        by_start[(size_t)i] = {keys[2 * i], i};
        by_end[(size_t)i] = {keys[2 * i + 1], i};
    }
    std::sort(by_start.begin(), by_start.end());
    std::sort(by_end.begin(), by_end.end());
    for (int64_t i = 1; i < n; ++i)
        if (by_start[(size_t)i].first == by_start[(size_t)i - 1].first || by_end[(size_t)i].first == by_end[(size_t)i - 1].first)
            return -1;
    // next[i]: the segment that starts where i ends; has_prev[i]: some segment ends where i starts
    std::vector<int64_t> next((size_t)n, -1);
    std::vector<uint8_t> has_prev((size_t)n, 0), used((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const auto it = std::lower_bound(by_start.begin(), by_start.end(), std::make_pair(keys[2 * i + 1], (int64_t)-1));
        if (it != by_start.end() && it->first == keys[2 * i + 1]) {
            next[(size_t)i] = it->second;
            has_prev[(size_t)it->second] = 1;
        }
    }
    int64_t at = 0, loops = 0;
    for (int pass = 0; pass < 2; ++pass) {   // open chains (from a start no segment ends on), then loops
        for (int64_t i = 0; i < n; ++i) {
            if (used[(size_t)i] || (pass == 0 && has_prev[(size_t)i])) continue;
            for (int64_t k = i; k >= 0 && !used[(size_t)k]; k = next[(size_t)k]) {
                used[(size_t)k] = 1;
                order[at++] = k;
            }
            closed[loops] = pass ? 1 : 0;
            loop_offsets[++loops] = at;
        }
    }
    return loops;
}

// ---------------------------------------------------------------------------------------------
namespace {

struct Builder {
    Program p{};
    int depth = 0, max_depth = 0;
    ObjectTables* tables = nullptr;   // receives the sdf_3d tables (null: such nodes are refused)

    int add_matrix(const float m[12]) {
        if (p.n_mats >= kMaxProgram) throw InputError("MP5 tree too large");
        float inv[12];
        if (!invert_matrix12(m, inv)) throw InputError("singular MP5 matrix");
        std::memcpy(p.mats[p.n_mats], inv, sizeof inv);
        return p.n_mats++;
    }
    int emit(OpCode op, int32_t type, int32_t mat, int32_t csg = -1) {
        if (p.n_instr >= kMaxProgram) throw InputError("MP5 tree too large");
        p.instr[p.n_instr] = Instr{(int16_t)op, (int16_t)type, (int16_t)mat, (int16_t)csg, -1, -1, -1, 0};
        return p.n_instr++;
    }

    static void matrix12(const Json& d, float m[12]) {   // getMatrix12 object_factory.hpp:21-30
        const Json* mj = d.find("matrix");
        if (!mj || mj->kind != Json::Array || mj->items.size() < 12)
            throw InputError("MP5 node needs a 12- or 16-entry \"matrix\"");
        for (int i = 0; i < 12; ++i) {
            float v;
            if (!mj->items[i].second.as_float(&v)) throw InputError("bad matrix entry");
            m[i] = v;
        }
    }

    // raw parameters (not inverted) for primitives that carry them (Instr::prm): ceil(n / 12)
    // consecutive rows of mats[], read as one float array
    int add_params(const float* v, int n) {
        const int rows = (n + 11) / 12;
        if (p.n_mats + rows > kMaxProgram) throw InputError("MP5 tree too large");
        const int first = p.n_mats;
        for (int r = 0; r < rows; ++r) {
            float row[12] = {};
            const int k = std::min(12, n - 12 * r);
            std::memcpy(row, v + 12 * r, sizeof(float) * (size_t)k);
            std::memcpy(p.mats[p.n_mats++], row, sizeof row);
        }
        return first;
    }

    // A "subtree" pushes exactly one value; it sees the parent's local point on top of the stack.
    void leaf(NodeType t, const float m[12], const float* prm = nullptr, int nprm = 0) {
        const int k = add_matrix(m);
        const int pr = prm ? add_params(prm, nprm) : 0;
        emit(OP_XFORM, t, k);
        push_point();
        const int pc = emit(OP_PRIM, t, k);
        p.instr[pc].prm = (int16_t)pr;
        pop_point();
    }

    // screw::getScrewParameters (screw.hpp:380-470) + constructor (:222-330), in float: outer =
    // |v| = 1 for v = (0,1,0), inner = outer / delta_ratio, r0 = inner / 2, delta = outer / 2 -
    // inner / 2, twist_rate = pitch.  ptree get_child/get throw on the missing keys (values unused).
    static void screw_params(const Json& d, float prm[3]) {
        for (const char* k : {"matrix", "v", "pitch", "profile", "end_type", "delta_ratio"})
            if (!d.find(k)) throw InputError(std::string("screw: missing \"") + k + "\"");
        float pitch, ratio;
        if (!d.get_float("pitch", &pitch) || !d.get_float("delta_ratio", &ratio))
            throw InputError("screw: pitch and delta_ratio must be numbers");
        const float outer = 1.0f, inner = outer / ratio;
        prm[0] = pitch;
        prm[1] = inner / 2;
        prm[2] = outer / 2 - inner / 2;
    }
    // half_plane constructor (half_plane.hpp:96-125): plane_vector / |plane_vector| in float, the
    // norm reduced a0 + (a1 + a2); prm = {unit vector, plane_point}
    static void half_plane_params(const float pv[3], const float pp[3], float prm[6]) {
        const float n = std::sqrt(pv[0] * pv[0] + (pv[1] * pv[1] + pv[2] * pv[2]));
        for (int k = 0; k < 3; ++k) {
            prm[k] = pv[k] / n;
            prm[3 + k] = pp[k];
        }
    }
    // tetrahedron (tetrahedron.hpp:20-128; getCorners object_factory.hpp:32-45, a missing corner
    // stays 0): corners moved by the forward node matrix (matrix_vector_product,
    // basic_functions.hpp:140-177), the four calculatePlaneCoefficients planes, each multiplied by
    // the sign (ROOT_TOLERANCE, configs.hpp:33) of its value at the opposite corner
    static void tetra_params(const Json& d, const float m[12], float out[16]) {
        float c[4][3] = {};
        if (const Json* cs = d.find("corners")) {
            if (cs->kind != Json::Array) throw InputError("tetrahedron: \"corners\" must be an array");
            for (size_t i = 0; i < cs->items.size() && i < 4; ++i) {
                const Json& cj = cs->items[i].second;
                for (size_t j = 0; j < cj.items.size() && j < 3; ++j)
                    if (!cj.items[j].second.as_float(&c[i][j])) throw InputError("tetrahedron: bad corner");
            }
        } else {
            throw InputError("tetrahedron: missing \"corners\"");
        }
        float p[4][3];
        for (int i = 0; i < 4; ++i)
            for (int r = 0; r < 3; ++r)
                p[i][r] = m[4 * r] * c[i][0] + m[4 * r + 1] * c[i][1] + m[4 * r + 2] * c[i][2] + m[4 * r + 3];
        auto coef = [](const float* P1, const float* P2, const float* P3, float* o) {
            const float x1 = P1[0], y1 = P1[1], z1 = P1[2], x2 = P2[0], y2 = P2[1], z2 = P2[2], x3 = P3[0], y3 = P3[1],
                        z3 = P3[2];
            o[0] = y1 * z2 - y1 * z3 - y2 * z1 + y2 * z3 + y3 * z1 - y3 * z2;
            o[1] = x1 * z3 - x1 * z2 + x2 * z1 - x2 * z3 - x3 * z1 + x3 * z2;
            o[2] = x1 * y2 - x1 * y3 - x2 * y1 + x2 * y3 + x3 * y1 - x3 * y2;
            o[3] = x1 * y3 * z2 - x1 * y2 * z3 + x2 * y1 * z3 - x2 * y3 * z1 - x3 * y1 * z2 + x3 * y2 * z1;
        };
        coef(p[1], p[2], p[3], out);
        coef(p[0], p[2], p[3], out + 4);
        coef(p[0], p[1], p[3], out + 8);
        coef(p[0], p[1], p[2], out + 12);
        const float tol = (float)(0.001 / 10.0);
        for (int k = 0; k < 4; ++k) {
            float* P = out + 4 * k;
            const float v = P[0] * p[k][0] + P[1] * p[k][1] + P[2] * p[k][2] + P[3];
            const float sg = (v > +tol) ? 1.0f : (v < -tol) ? -1.0f : 0.0f;   // sign(), basic_functions.hpp:22-31
            for (int j = 0; j < 4; ++j) P[j] *= sg;
        }
    }
    // meta_ball_Rydgard (meta_balls_Rydgard.hpp:27-60): 4 blobs, scale 1; ball centres in double
    // (libm sin / cos) stored to float; strength 1.2 / ((sqrt(4) - 1) / 4 + 1), subtract 12
    static void metaball_params(const Json& d, float out[20]) {
        float time = 0.1f;   // get<REAL>("time", 0.1)
        if (d.find("time") && !d.get_float("time", &time)) throw InputError("meta_balls: bad \"time\"");
        const int numblobs = 4;
        for (int i = 0; i < numblobs; ++i) {
            const float x0 = 0.5f, y0 = 0.5f, z0 = 0.5f, D = 1;
            const float ballx = (float)(std::sin(i + 1.26 * time * (1.03 + 0.5 * std::cos(0.21 * i))) * 0.27 * D + 0.5 - x0);
            const float bally = (float)(std::abs(std::cos(i + 1.12 * time * std::cos(1.22 + 0.1424 * i))) * 0.77 * D - y0);
            const float ballz = (float)(std::cos(i + 1.32 * time * 0.1 * std::sin((0.92 + 0.53 * i))) * 0.27 * D + 0.5 - z0);
            const float subtract = 12;
            const float strength = (float)(1.2 / ((std::sqrt((double)numblobs) - 1) / 4 + 1));
            const float v[5] = {ballx, bally, ballz, strength, subtract};
            std::memcpy(out + 5 * i, v, sizeof v);
        }
    }
    // extrusion(eye, size) (extrusion.hpp:61-94) with convex_polygon::update_inner_data
    // (2d/GDT/convex_polygon.hpp:77-93): regular size-gon of radius 0.5 from (0, 0.5),
    // polarToCartesian (basic_functions.hpp:33-36) through std::cos/sin(float); 1/d in double
    static int extrusion_params(const Json& d, float* out) {
        float fs;
        if (!d.get_float("size", &fs)) throw InputError("extrusion: missing \"size\"");
        if (!(fs > -2147483648.f && fs < 2147483648.f)) throw InputError("extrusion: Invalid size");   // no int holds it
        const int size = (int)fs;
        if (size < 3) throw InputError("extrusion: Invalid size");
        if (size > 40) throw InputError("extrusion: size above 40 is not supported");
        const float PI = (float)3.141592653589793238463;   // basic_functions.hpp:8
        const float rot = 2 * PI / size;
        std::vector<float> cx{0.f}, cy{0.5f};
        const float radius = 0.5f;
        for (int i = 1; i < size; ++i) {
            const float theta = (float)(PI / 2.0 + i * rot);
            cx.push_back(radius * std::cos(theta));
            cy.push_back(radius * std::sin(theta));
        }
        out[0] = (float)size;
        for (int i = 0; i < size; ++i) {
            const int j = (i < size - 1) ? i + 1 : 0;
            const float dx = cx[j] - cx[i], dy = cy[j] - cy[i];
            const float dd = std::sqrt(dx * dx + dy * dy);
            const float dinv = (float)((dd > 0.00000001) ? 1.0 / dd : 0.0);
            const float nx = +dy * dinv, ny = -dx * dinv;
            out[1 + 3 * i] = nx;
            out[2 + 3 * i] = ny;
            out[3 + 3 * i] = cx[i] * nx + cy[i] * ny;
        }
        return 1 + 3 * size;
    }

    // sdf_3d (object_factory.hpp:352-395, sdf_3d.hpp:73-102): sizes, grid_size, origin and the "sdf"
    // array, flat index x + y size_x + z size_x size_y as in cube.hpp.  Validates the node, appends
    // its zero-padded table to `tables` and lays out its arena section (host.hpp ObjectTables).
    void sdf3d_params(const Json& d, float prm[kSdfParams]) {
        (void)d.get_int("id", 0);   // read, otherwise unused
        int size[3];
        const char* size_keys[3] = {"size_x", "size_y", "size_z"};
        for (int k = 0; k < 3; ++k) {
            if (!d.find(size_keys[k])->as_int(&size[k]))
                throw InputError(std::string("sdf_3d: \"") + size_keys[k] + "\" must be an integer");
            if (size[k] < kSdfMinSize || size[k] > kSdfMaxSize)
                throw InputError(std::string("sdf_3d: \"") + size_keys[k] + "\" must be in [2, 512]");
        }
        const int64_t N = (int64_t)size[0] * size[1] * size[2];
        if (N > kSdfMaxEntries) throw InputError("sdf_3d: size_x * size_y * size_z exceeds 2^22 entries");
        float gs, org[3];
        if (!d.get_float("grid_size", &gs) || !std::isfinite(gs) || !(gs > 0.f))
            throw InputError("sdf_3d: \"grid_size\" must be a finite number > 0");
        const char* org_keys[3] = {"origin_x", "origin_y", "origin_z"};
        for (int k = 0; k < 3; ++k)
            if (!d.get_float(org_keys[k], &org[k]) || !std::isfinite(org[k]))
                throw InputError(std::string("sdf_3d: \"") + org_keys[k] + "\" must be a finite number");
        // the largest cell index the point function computes, (int)((X - o) / gs) at the box's far
        // face X = o + gs size (monotone in X), in the device's float operations: it must stay at
        // size, the last index the padding covers (a grid_size far below the origin's rounding
        // step would pass it)
        for (int k = 0; k < 3; ++k) {
            const float far = org[k] + gs * (float)size[k];
            const float cell = (far - org[k]) / gs;
            if (!std::isfinite(far) || !(cell < (float)(size[k] + 1)))
                throw InputError(std::string("sdf_3d: \"grid_size\" is too small against \"") + org_keys[k] +
                                 "\" (the table box does not resolve in float)");
        }
        const Json* sdf = d.find("sdf");
        if (sdf->kind != Json::Array) throw InputError("sdf_3d: \"sdf\" must be an array");
        if ((int64_t)sdf->items.size() != N)
            throw InputError("sdf_3d: \"sdf\" holds " + std::to_string(sdf->items.size()) + " values, size_x * size_y * size_z is " +
                             std::to_string(N));
        if ((int)tables->nodes.size() >= kSdfMaxNodes) throw InputError("sdf_3d: more than 8 sdf_3d nodes in one object");

        SdfTable T{};
        T.sx = (uint32_t)size[0]; T.sy = (uint32_t)size[1]; T.sz = (uint32_t)size[2];
        const uint32_t sxy = T.sx * T.sy;
        T.level0 = T.sx + T.sy * T.sx + T.sz * sxy + 1;          // flat indices of the cells 0 .. size per axis
        T.padded = (T.level0 + 1 + T.sx + sxy + 1) & ~1u;         // + the eight reads' reach, kept even (float2 alignment)
        T.data_off = tables->data.size();
        tables->data.resize(T.data_off + T.padded, 0.f);
        float* tab = tables->data.data() + T.data_off;
        float vmin = 0.f, vmax = 0.f;                             // the padding's zeros are readable
        for (int64_t i = 0; i < N; ++i) {
            float v;
            if (!sdf->items[(size_t)i].second.as_float(&v) || !std::isfinite(v))
                throw InputError("sdf_3d: \"sdf\"[" + std::to_string(i) + "] is not a finite number");
            tab[i] = v;
            vmin = v < vmin ? v : vmin;
            vmax = v > vmax ? v : vmax;
        }
        uint32_t smax = std::max(T.sx, std::max(T.sy, T.sz)), top = 0;
        while ((smax >> top) > 1) ++top;
        T.n_levels = top + 1;
        size_t off = tables->nodes.empty() ? (size_t)kArenaRabbitFloats : tables->arena_floats;
        T.tab_off = (uint32_t)off;
        off += T.padded;
        for (uint32_t L = 0; L < T.n_levels; ++L) {
            T.lvl_off[L] = (uint32_t)off;
            const size_t entries = L == 0 ? (size_t)T.level0
                                          : (size_t)((T.sx >> L) + 1) * ((T.sy >> L) + 1) * ((T.sz >> L) + 1);
            off += 2 * entries;
        }
        tables->arena_floats = off;
        tables->nodes.push_back(T);

        auto bits = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
        std::memset(prm, 0, sizeof(float) * kSdfParams);
        prm[SDF_SX] = (float)T.sx; prm[SDF_SY] = (float)T.sy; prm[SDF_SZ] = (float)T.sz;
        prm[SDF_GS] = gs; prm[SDF_OX] = org[0]; prm[SDF_OY] = org[1]; prm[SDF_OZ] = org[2];
        prm[SDF_VMIN] = vmin; prm[SDF_VMAX] = vmax;
        prm[SDF_TAB] = bits(T.tab_off);
        prm[SDF_LEVELS] = (float)T.n_levels;
        for (uint32_t L = 0; L < T.n_levels; ++L) prm[SDF_LVL0 + L] = bits(T.lvl_off[L]);
    }

    static void vec3(const Json& d, const char* key, float out[3]) {
        const Json* a = d.find(key);
        if (!a || a->kind != Json::Array || a->items.size() < 3) throw InputError(std::string("half_plane: bad \"") + key + "\"");
        for (int k = 0; k < 3; ++k)
            if (!a->items[k].second.as_float(&out[k])) throw InputError(std::string("half_plane: bad \"") + key + "\"");
    }
    void push_point() { if (++depth > max_depth) max_depth = depth; if (depth >= kMaxDepth) throw InputError("MP5 tree too deep"); }
    void pop_point() { --depth; }

    // node = XFORM(m); child a; child b; CSG(t).  Each operand subtree starts with its own XFORM,
    // which records where the subtree ends so a pruned operand can be skipped in one jump.
    template <class A, class B>
    void csg(NodeType t, const float m[12], A&& a, B&& b) {
        const int k = add_matrix(m);
        const int id = p.n_csg++;
        emit(OP_XFORM, t, k);
        push_point();
        const int a0 = p.n_instr;
        a();
        mark_operand(a0, id, 0);
        const int b0 = p.n_instr;
        b();
        mark_operand(b0, id, 1);
        emit(OP_CSG, t, k, id);
        pop_point();
    }
    void mark_operand(int start, int csg_id, int child) {
        p.instr[start].skip_csg = (int16_t)csg_id;
        p.instr[start].skip_child = (int16_t)child;
        p.instr[start].skip_to = (int16_t)p.n_instr;
    }

    void node(const Json& d, bool ignore) {
        static const float eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        std::string t = d.get_string("type", "");
        float m[12];
        struct { const char* name; NodeType t; } prims[] = {
            {"implicit_double_mushroom", NT_DMUSHROOM},        // object_factory.hpp:86-100
            {"icube", NT_CUBE}, {"cube", NT_CUBE},             // :110-119 (rabbit SDF, F3)
            {"icylinder", NT_CYLINDER}, {"cylinder", NT_CYLINDER},  // :121-132
            {"iellipsoid", NT_ELLIPSOID}, {"ellipsoid", NT_ELLIPSOID},  // :134-143
            {"icone", NT_CONE}, {"cone", NT_CONE},             // :144-152
            {"iheart", NT_HEART},                              // :153-162
            {"itorus", NT_TORUS},                              // :163-173
        };
        for (auto& pr : prims)
            if (t == pr.name) {
                matrix12(d, m);
                if (ignore) std::memcpy(m, eye, sizeof m);
                leaf(pr.t, m);
                return;
            }
        if (t == "Union") {   // :537-580: left-deep chain, identity on the intermediate unions
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            const Json* ch = d.find("children");
            if (!ch || ch->kind != Json::Array || ch->items.size() < 2)
                throw InputError("Union needs at least two children");
            union_chain(*ch, (int)ch->items.size() - 1, m);
            return;
        }
        if (t == "Intersection" || t == "Difference") {   // :581-653, binary
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            const Json* ch = d.find("children");
            if (!ch || ch->kind != Json::Array || ch->items.size() < 2)
                throw InputError(t + " needs two children");
            csg(t == "Intersection" ? NT_INTERSECTION : NT_DIFFERENCE, m,
                [&] { node(ch->items[0].second, false); }, [&] { node(ch->items[1].second, false); });
            return;
        }
        if (t == "screw" || t == "inf_screw" || t == "screw_diff_two_plane") {
            float prm[3];
            screw_params(d, prm);
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            if (t == "inf_screw") {   // object_factory.hpp:189-215: the screw under its own matrix
                leaf(NT_SCREW, m, prm, 3);
                return;
            }
            if (t == "screw") {       // :304-351: subtract(screw(identity), top_bottom_lid)
                csg(NT_DIFFERENCE, m, [&] { leaf(NT_SCREW, eye, prm, 3); }, [&] { leaf(NT_LID, eye); });
                return;
            }
            // :216-302: subtract(subtract(screw, half_plane z >= 0.25), half_plane z <= -0.25)
            const float up[3] = {0, 0, 1}, upp[3] = {0, 0, 0.25f}, dn[3] = {0, 0, -1}, dnp[3] = {0, 0, -0.25f};
            float top[6], bot[6];
            half_plane_params(up, upp, top);
            half_plane_params(dn, dnp, bot);
            csg(NT_DIFFERENCE, m,
                [&] { csg(NT_DIFFERENCE, eye, [&] { leaf(NT_SCREW, eye, prm, 3); }, [&] { leaf(NT_HALF_PLANE, eye, top, 6); }); },
                [&] { leaf(NT_HALF_PLANE, eye, bot, 6); });
            return;
        }
        if (t == "screw_gradient_wrong") {
            // :435-479: inf_top_bot_bound(T, screw(T)) -- the screw under the JSON matrix T (no
            // ignore_root_matrix here) bounded by the lid at the same x' = T^-1 x.  The node's
            // gradient applies T^-T twice (inf_top_bot_bound.hpp:142-166 over screw.hpp:476-486),
            // so the primitive carries a copy of the inverse
            float prm[24] = {};
            screw_params(d, prm);
            matrix12(d, m);
            if (!invert_matrix12(m, prm + 12)) throw InputError("singular MP5 matrix");
            leaf(NT_SCREW_TBB, m, prm, 24);
            return;
        }
        if (t == "top_bottom_lid") {   // :480-506: the matrix is read (get_child) and never applied
            matrix12(d, m);
            leaf(NT_LID, eye);
            return;
        }
        if (t == "half_plane") {       // :396-434
            float pv[3], pp[3], prm[6];
            vec3(d, "plane_vector", pv);
            vec3(d, "plane_point", pp);
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            half_plane_params(pv, pp, prm);
            leaf(NT_HALF_PLANE, m, prm, 6);
            return;
        }
        if (t == "tetrahedron") {      // :175-188: the corners are moved, the object itself is not
            float prm[16];
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            tetra_params(d, m, prm);
            leaf(NT_TETRA, eye, prm, 16);
            return;
        }
        if (t == "meta_balls") {       // :654-673
            float prm[20];
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            metaball_params(d, prm);
            leaf(NT_METABALLS, m, prm, 20);
            return;
        }
        if (t == "extrusion") {        // :674-731: subtract(extrusion(eye, size), top_bottom_lid)
            float prm[1 + 3 * 40];
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            const int n = extrusion_params(d, prm);
            csg(NT_DIFFERENCE, m, [&] { leaf(NT_EXTRUSION, eye, prm, n); }, [&] { leaf(NT_LID, eye); });
            return;
        }
        if (t == "sdf_3d") {           // :352-395, sdf_3d.hpp:73-102: the table is read from the node
            // a node without the table fields is the reference's by-id form (the table fetched by
            // JavaScript): outside the implemented families, as before
            std::string missing;
            for (const char* k : {"size_x", "size_y", "size_z", "grid_size", "origin_x", "origin_y", "origin_z", "sdf"})
                if (!d.find(k)) missing += std::string(missing.empty() ? "" : ", ") + "\"" + k + "\"";
            if (!missing.empty())
                throw InputError("MP5 type \"sdf_3d\" is outside the implemented node families: the node carries no " +
                                 missing + " (a table fetched by id is not supported)");
            // (object streams pass no table receiver: their programs travel without table arenas)
            if (!tables) throw InputError("MP5 type \"sdf_3d\" is not supported in an object stream (implisolid_batch_create)");
            matrix12(d, m);
            if (ignore) std::memcpy(m, eye, sizeof m);
            float prm[kSdfParams];
            sdf3d_params(d, prm);
            leaf(NT_SDF3D, m, prm, kSdfParams);
            return;
        }
        static const char* unsupported[] = {"sdf_3d", "rawjscode"};
        for (auto* u : unsupported)
            if (t == u) throw InputError("MP5 type \"" + t + "\" is outside the implemented node families");
        throw InputError("Invalid object you asked for: \"" + t + "\"");
    }

    // union of children[0..k] = U(union of children[0..k-1], children[k]) with matrix m at the top
    void union_chain(const Json& ch, int k, const float m[12]) {
        static const float eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        if (k == 0) {
            node(ch.items[0].second, false);
            return;
        }
        csg(NT_UNION, m, [&] { union_chain(ch, k - 1, eye); }, [&] { node(ch.items[k].second, false); });
    }
};

}  // namespace

bool ObjectTables::same(const ObjectTables& o) const {
    if (nodes.size() != o.nodes.size() || arena_floats != o.arena_floats || data.size() != o.data.size()) return false;
    for (size_t i = 0; i < nodes.size(); ++i) {
        const SdfTable &a = nodes[i], &b = o.nodes[i];
        if (a.sx != b.sx || a.sy != b.sy || a.sz != b.sz || a.tab_off != b.tab_off || a.data_off != b.data_off) return false;
    }
    return data.empty() || std::memcmp(data.data(), o.data.data(), data.size() * sizeof(float)) == 0;
}

Program compile_mp5(const Json& shape, bool ignore_root_matrix, ObjectTables* tables) {
    Builder b;
    if (tables) *tables = ObjectTables{};
    b.tables = tables;
    b.node(shape, ignore_root_matrix);
    b.p.max_depth = b.max_depth + 1;
    for (int i = 0; i < b.p.n_instr; ++i) {   // XFORM patterns (program.hpp XformPattern)
        Instr& I = b.p.instr[i];
        if (I.op != OP_XFORM) continue;
        const float* m = b.p.mats[I.mat];
        bool diag = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                const float v = m[4 * r + c];
                uint32_t bits;
                std::memcpy(&bits, &v, 4);
                if (!std::isfinite(v)) diag = false;
                else if (c == 3 && bits == 0x80000000u) diag = false;   // a -0 translation
                else if (c != 3 && c != r && v != 0.f) diag = false;
            }
        I.type = diag ? XF_DIAG : XF_GENERIC;
    }
    return b.p;
}

Program compile_mp5(const char* shape_json, bool ignore_root_matrix, ObjectTables* tables) {
    Json d;
    try {
        d = Json::parse(shape_json);
    } catch (const JsonError& e) {
        throw InputError(e.what());
    }
    return compile_mp5(d, ignore_root_matrix, tables);
}

// the largest resolution the settings parser accepts (the reference's dim_t, polygoniser_settings.hpp)
constexpr int kMaxResolution = 65535;

SlabRange slab_range(int R, int z0, int z1) {
    if (R < 1 || R > kMaxResolution) throw InputError("slab_range: resolution out of range");
    const int layers = (R + 5) - 3;   // cell layers 1 .. res-3
    if (z0 < 1 || z1 <= z0 || z1 > layers + 1) throw InputError("slab_range: bad layer range");
    SlabRange r{z0, z1, z0 > 1 ? 1 : 0};
    // 32-bit indexing of one slab (mc_types.hpp / mc_device.hpp): the cell id L of a slab's cells
    // (halo layer included) is a uint32, and so are vertex ids, face rows and the MC counters.
    const int64_t m = (int64_t)R + 2, cells = m * m * (int64_t)(z1 - z0 + r.halo);
    if (cells >= (int64_t)1 << 32)
        throw InputError("slab of " + std::to_string(cells) + " cells exceeds the 2^32-cell limit of one slab (R = " +
                         std::to_string(R) + "): split the grid over more Z-slabs");
    return r;
}

SlabRange slab_partition(int R, int rank, int nranks) {
    if (R < 1 || R > kMaxResolution || nranks < 1 || rank < 0 || rank >= nranks) throw InputError("slab_partition: bad arguments");
    const int layers = (R + 5) - 3;   // cell layers 1 .. res-3
    if (nranks > layers) throw InputError("slab_partition: more slabs than cell layers");
    const int base = layers / nranks, extra = layers % nranks;
    const int z0 = 1 + rank * base + (rank < extra ? rank : extra);
    return slab_range(R, z0, z0 + base + (rank < extra ? 1 : 0));
}

void GlibcRand::seed_(unsigned seed) {   // srandom_r (random_r.c:161-196)
    int32_t word = seed == 0 ? 1 : (int32_t)seed;
    r_[0] = (uint32_t)word;
    for (int i = 1; i < 31; ++i) {        // 16807 * word mod (2^31 - 1), Schrage's method
        const int32_t hi = word / 127773, lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r_[i] = (uint32_t)word;
    }
    head_ = 3;                            // fptr = &state[SEP_3] holds the oldest term
    for (int i = 0; i < 310; ++i) next();
}

int32_t GlibcRand::next() {               // random_r (random_r.c:353-394): *fptr += *rptr
    int b = head_ + 28;
    if (b >= 31) b -= 31;
    const uint32_t v = r_[head_] + r_[b];
    r_[head_] = v;
    if (++head_ == 31) head_ = 0;
    return (int32_t)(v >> 1);
}

void GlibcRand::extended_window(uint32_t out[61]) const {
    for (int j = 0; j < 31; ++j) out[j] = r_[(head_ + j) % 31];
    for (int j = 31; j < 61; ++j) out[j] = out[j - 31] + out[j - 3];
}

void GlibcRand::skip(uint64_t n) {
    uint32_t c[31], x[61];
    rand_jump_poly(n, c);
    extended_window(x);
    for (int j = 0; j < 31; ++j) {
        uint32_t acc = 0;
        for (int i = 0; i < 31; ++i) acc += c[i] * x[i + j];
        r_[j] = acc;
    }
    head_ = 0;
}

void rand_poly_mulmod(const uint32_t a[31], const uint32_t b[31], uint32_t out[31]) {
    uint32_t p[61] = {};
    for (int i = 0; i < 31; ++i)
        for (int j = 0; j < 31; ++j) p[i + j] += a[i] * b[j];
    for (int k = 60; k >= 31; --k) {      // z^k = z^(k-3) + z^(k-31)
        p[k - 3] += p[k];
        p[k - 31] += p[k];
    }
    for (int i = 0; i < 31; ++i) out[i] = p[i];
}

void rand_jump_poly(uint64_t n, uint32_t c[31]) {
    uint32_t base[31] = {}, r[31] = {};
    base[1] = 1;   // z
    r[0] = 1;
    for (; n; n >>= 1) {
        if (n & 1) rand_poly_mulmod(r, base, r);
        rand_poly_mulmod(base, base, base);
    }
    for (int i = 0; i < 31; ++i) c[i] = r[i];
}

GlibcRand& process_rand() {
    static GlibcRand g(1);
    return g;
}

}  // namespace impli
