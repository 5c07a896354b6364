// ply_options.h -- what the drop-in host does to the fused points before it writes APD.ply (the --ply-* flags but --ply-normals,
// which is a field of apd_fusion_options): the options, declared here once for host/main.cpp, which fills them, and
// host/fusion.cpp, which applies them, and the reading of the flags' values.  No device call and no globals in here:
// tests/test_ply_option_values.py runs the same reading through host_capi.cpp on a machine without a device.
#ifndef APD_MI355X_HOST_PLY_OPTIONS_H_
#define APD_MI355X_HOST_PLY_OPTIONS_H_

#include <cerrno>
#include <cstdlib>
#include <string>
#include <vector>

// The steps are applied in the order of the fields: mean, voxel, stat, radius, component, smooth, normals, render, register, align, align
// to planes; APD.ply is then written, and score comes last.
struct PlyOptions {
    bool vis = false;                 // --ply-vis: APD/APD.ply.vis beside APD.ply (apd_points_write_vis)
    bool mean = false;                // --ply-mean: APD.ply (and APD.ply.vis) of the points averaged over their agreeing views (apd_points_average)
    float voxel = 0.0f;               // --ply-voxel SIZE: APD.ply (and APD.ply.vis) of the points merged per cell of that size (apd_points_merge_voxels); 0: off
    float stat_radius = 0.0f;         // --ply-stat-filter RADIUS,K,RATIO: APD.ply (and APD.ply.vis) of the points whose mean distance to their K
    unsigned stat_k = 0;              // nearest neighbours within RADIUS is at most mean + RATIO * deviation (apd_points_remove_statistical);
    float stat_ratio = 0.0f;          // radius 0: off
    float radius = 0.0f;              // --ply-radius-filter RADIUS,MIN: APD.ply (and APD.ply.vis) of the points with at least MIN others within
    unsigned radius_min = 0;          // RADIUS (apd_points_remove_sparse); radius 0: off
    float component_radius = 0.0f;    // --ply-component-filter RADIUS,MIN: APD.ply (and APD.ply.vis) of the points whose connected component within
    unsigned component_min = 0;       // RADIUS has at least MIN points (apd_points_remove_small_components); radius 0: off
    float smooth_radius = 0.0f;       // --ply-smooth RADIUS,MIN[,ITERATIONS]: the points of APD.ply with each position projected on the weighted plane of
    unsigned smooth_min = 0;          // its neighbourhood within RADIUS where it has at least MIN others there, ITERATIONS (1 .. 16, default 1) times
    unsigned smooth_iterations = 1;   // (apd_points_with_smoothed_positions); radius 0: off
    float normals_radius = 0.0f;      // --ply-estimate-normals RADIUS,MIN: the points of APD.ply with normals estimated from the neighbourhood within
    unsigned normals_min = 0;         // RADIUS of each point that has at least MIN others there (apd_points_with_estimated_normals); radius 0: off
    int render_splat = -1;            // --ply-render-vis SPLAT,TOL: APD.ply.vis (the flag implies --ply-vis) lists per point the views that see it when the
    float render_tolerance = 0.0f;    // cloud is drawn into them with footprints of SPLAT (apd_points_rendered_visibility); splat -1: off
    std::string register_truth;       // --ply-register TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]]: the points of APD.ply moved onto the cloud of TRUTH.ply from
    float register_radius = 0.0f;     // any start (apd_points_register with descriptors at RADIUS and inliers within DISTANCE, apd_points_transformed):
    float register_distance = 0.0f;   // one printed line and APD.ply.register; empty: off
    unsigned register_trials = 4096;
    unsigned long long register_seed = 0;
    std::string align_truth;          // --ply-align TRUTH.ply,RADIUS[,ITERATIONS[,scale]]: the points of APD.ply moved onto the cloud of TRUTH.ply by ICP
    float align_radius = 0.0f;        // within RADIUS (apd_points_align, apd_points_transformed): one printed line and APD.ply.align; empty: off
    unsigned align_iterations = 16;
    bool align_scale = false;
    std::string planes_truth;         // --ply-align-planes TRUTH.ply,RADIUS[,ITERATIONS]: the points of APD.ply moved onto the tangent planes of the cloud of
    float planes_radius = 0.0f;       // TRUTH.ply, which must hold nx ny nz, by point-to-plane ICP within RADIUS (apd_points_align_planes,
    unsigned planes_iterations = 16;  // apd_points_transformed): one printed line and APD.ply.align_planes; empty: off
    std::string score_truth;          // --ply-score TRUTH.ply,TAU: the points of APD.ply scored against the cloud of TRUTH.ply at threshold TAU
    float score_threshold = 0.0f;     // (apd_points_score): one printed line and APD.ply.score; empty: off

    // APD.ply is written from the points after the fusion, not by it
    bool from_points() const
    {
        return mean || voxel > 0.0f || stat_radius > 0.0f || radius > 0.0f || component_radius > 0.0f || smooth_radius > 0.0f || normals_radius > 0.0f ||
               render_splat >= 0 || !register_truth.empty() || !align_truth.empty() || !planes_truth.empty() ||
               !score_truth.empty();
    }
};

namespace ply_value {

// The value split at its first `cuts` commas (what follows the last of them stays whole), or from the right at its last `cuts`
// commas for the values that start with a file's name, which may hold commas itself and must not be empty.  Empty when the value
// has fewer commas.
inline std::vector<std::string> Split(const std::string &value, size_t cuts, bool from_right = false)
{
    std::vector<size_t> at;
    for (size_t c = from_right ? value.rfind(',') : value.find(','); c != std::string::npos && at.size() < cuts && !(from_right && c == 0);
         c = from_right ? value.rfind(',', c - 1) : value.find(',', c + 1)) {
        at.insert(from_right ? at.begin() : at.end(), c);
    }
    std::vector<std::string> token;
    for (size_t k = 0; at.size() == cuts && k <= cuts; ++k) {
        const size_t from = k == 0 ? 0 : at[k - 1] + 1;
        token.push_back(value.substr(from, k == cuts ? std::string::npos : at[k] - from));
    }
    return token;
}

// a non-negative finite number that fills the whole token
inline bool Real(const std::string &text, float &dst)
{
    char *end = nullptr;
    const float f = strtof(text.c_str(), &end);
    if (end == text.c_str() || *end != '\0' || !(f >= 0.0f) || f > 3.402823466e+38f) {
        return false;
    }
    dst = f;
    return true;
}

// a radius: a positive number whose square is positive and finite too (it is the cell size of a grid, and distances are compared squared)
inline bool Radius(const std::string &text, float &dst)
{
    float r = 0.0f;
    if (!Real(text, r) || !(r * r > 0.0f) || r * r > 3.402823466e+38f) {
        return false;
    }
    dst = r;
    return true;
}

// a count of lo .. hi: digits only
inline bool Count(const std::string &text, unsigned long long lo, unsigned long long hi, unsigned long long &dst)
{
    char *end = nullptr;
    errno = 0;
    const unsigned long long n = strtoull(text.c_str(), &end, 10);
    if (text.empty() || text.find_first_not_of("0123456789") != std::string::npos || *end != '\0' || errno != 0 || n < lo || n > hi) {
        return false;
    }
    dst = n;
    return true;
}

// RADIUS,MIN of --ply-radius-filter, --ply-component-filter and --ply-estimate-normals
inline bool RadiusAndCount(const std::string &value, unsigned long long lo, unsigned long long hi, float &radius, unsigned &count)
{
    const std::vector<std::string> t = Split(value, 1);
    float r = 0.0f;
    unsigned long long n = 0;
    if (t.empty() || !Count(t[1], lo, hi, n) || !Radius(t[0], r)) {
        return false;
    }
    radius = r;
    count = (unsigned)n;
    return true;
}

}  // namespace ply_value

// The --ply-* flags that take a value: what a bad value is told, and the reading of a good one into the options (which a bad one
// leaves as they are).
struct PlyFlag {
    const char *name, *expects;
    bool (*read)(const std::string &value, PlyOptions &o);
};

inline const PlyFlag *FindPlyFlag(const std::string &name)
{
    using namespace ply_value;
    static const PlyFlag flags[] = {
        {"--ply-voxel", "a positive number",
         [](const std::string &value, PlyOptions &o) {
             float size = 0.0f;
             if (!Real(value, size) || !(size > 0.0f)) {
                 return false;
             }
             o.voxel = size;
             return true;
         }},
        {"--ply-stat-filter", "RADIUS,K,RATIO, a positive number, a count of 1 .. 64 and a number",
         [](const std::string &value, PlyOptions &o) {
             const std::vector<std::string> t = Split(value, 2);
             if (t.empty()) {
                 return false;
             }
             char *end = nullptr;
             const float ratio = strtof(t[2].c_str(), &end);   // any finite number, zero and negative included
             float r = 0.0f;
             unsigned long long k = 0;
             if (end == t[2].c_str() || *end != '\0' || !(ratio >= -3.402823466e+38f && ratio <= 3.402823466e+38f) || !Count(t[1], 1, 64, k) || !Radius(t[0], r)) {
                 return false;
             }
             o.stat_radius = r;
             o.stat_k = (unsigned)k;
             o.stat_ratio = ratio;
             return true;
         }},
        {"--ply-radius-filter", "RADIUS,MIN, a positive number and a count",
         [](const std::string &value, PlyOptions &o) { return RadiusAndCount(value, 0, 0xffffffffull, o.radius, o.radius_min); }},
        {"--ply-component-filter", "RADIUS,MIN, a positive number and a count",
         [](const std::string &value, PlyOptions &o) { return RadiusAndCount(value, 0, 0xffffffffull, o.component_radius, o.component_min); }},
        {"--ply-smooth", "RADIUS,MIN[,ITERATIONS], a positive number, a count of 2 or more and a count of 1 .. 16",
         [](const std::string &value, PlyOptions &o) {
             std::vector<std::string> t = Split(value, 2);
             if (t.empty()) {
                 t = Split(value, 1);
                 t.push_back("1");
             }
             float r = 0.0f;
             unsigned long long k = 0, n = 0;
             if (t.size() != 3 || !Count(t[1], 2, 0x7fffffffull, k) || !Count(t[2], 1, 16, n) || !Radius(t[0], r)) {
                 return false;
             }
             o.smooth_radius = r;
             o.smooth_min = (unsigned)k;
             o.smooth_iterations = (unsigned)n;
             return true;
         }},
        {"--ply-estimate-normals", "RADIUS,MIN, a positive number and a count of 2 or more",
         [](const std::string &value, PlyOptions &o) { return RadiusAndCount(value, 2, 0x7fffffffull, o.normals_radius, o.normals_min); }},
        {"--ply-render-vis", "SPLAT,TOL, a count of 0 .. 8 and a non-negative number",
         [](const std::string &value, PlyOptions &o) {
             const std::vector<std::string> t = Split(value, 1);
             float tolerance = 0.0f;
             unsigned long long splat = 0;
             if (t.empty() || t[0].size() != 1 || !Count(t[0], 0, 8, splat) || !Real(t[1], tolerance)) {   // one digit: "08" is no splat
                 return false;
             }
             o.render_splat = (int)splat;
             o.render_tolerance = tolerance;
             o.vis = true;
             return true;
         }},
        {"--ply-register", "TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]], a file, two positive numbers, a count of 1 .. 65536 and a seed",
         [](const std::string &value, PlyOptions &o) {
             // read from the right, since the file's name may hold commas: the longest tail of four, three or two tokens that is
             // RADIUS,DISTANCE[,TRIALS[,SEED]]
             for (size_t tokens = 4; tokens >= 2; --tokens) {
                 const std::vector<std::string> t = Split(value, tokens, true);
                 float r = 0.0f, d = 0.0f;
                 unsigned long long trials = 4096, seed = 0;
                 if (!t.empty() && Radius(t[1], r) && Radius(t[2], d) && (tokens < 3 || Count(t[3], 1, 65536, trials)) &&
                     (tokens < 4 || Count(t[4], 0, ~0ull, seed))) {
                     o.register_truth = t[0];
                     o.register_radius = r;
                     o.register_distance = d;
                     o.register_trials = (unsigned)trials;
                     o.register_seed = seed;
                     return true;
                 }
             }
             return false;
         }},
        {"--ply-align", "TRUTH.ply,RADIUS[,ITERATIONS[,scale]], a file, a positive number and a count of 1 .. 64",
         [](const std::string &value, PlyOptions &o) {
             // read from the right, since the file's name may hold commas: [,scale], then [,ITERATIONS] when what stands before it is a
             // radius too, then ,RADIUS
             const bool scale = value.size() > 6 && value.compare(value.size() - 6, 6, ",scale") == 0;
             const std::string rest = scale ? value.substr(0, value.size() - 6) : value;
             std::vector<std::string> t = Split(rest, 2, true);
             float r = 0.0f;
             unsigned long long iterations = 16;
             if (t.empty() || !Count(t[2], 1, 64, iterations) || !Radius(t[1], r)) {
                 iterations = 16;
                 t = Split(rest, 1, true);
                 if (t.empty() || !Radius(t[1], r)) {
                     return false;
                 }
             }
             o.align_truth = t[0];
             o.align_radius = r;
             o.align_iterations = (unsigned)iterations;
             o.align_scale = scale;
             return true;
         }},
        {"--ply-align-planes", "TRUTH.ply,RADIUS[,ITERATIONS], a file with nx ny nz, a positive number and a count of 1 .. 64",
         [](const std::string &value, PlyOptions &o) {
             // read from the right, as --ply-align: [,ITERATIONS] when what stands before it is a radius too, then ,RADIUS
             std::vector<std::string> t = Split(value, 2, true);
             float r = 0.0f;
             unsigned long long iterations = 16;
             if (t.empty() || !Count(t[2], 1, 64, iterations) || !Radius(t[1], r)) {
                 iterations = 16;
                 t = Split(value, 1, true);
                 if (t.empty() || !Radius(t[1], r)) {
                     return false;
                 }
             }
             o.planes_truth = t[0];
             o.planes_radius = r;
             o.planes_iterations = (unsigned)iterations;
             return true;
         }},
        {"--ply-score", "TRUTH.ply,TAU, a file and a positive number",
         [](const std::string &value, PlyOptions &o) {
             const std::vector<std::string> t = Split(value, 1, true);
             if (t.empty() || !Radius(t[1], o.score_threshold)) {
                 return false;
             }
             o.score_truth = t[0];
             return true;
         }},
    };
    for (const PlyFlag &f : flags) {
        if (name == f.name) {
            return &f;
        }
    }
    return nullptr;
}

// Reads the value of a --ply-* flag that takes one into `o`.  Returns an empty string, or what the command line is told about
// a bad value (`o` is then as it was).  `flag` must be one that FindPlyFlag knows.
inline std::string ParsePlyOption(const std::string &flag, const std::string &value, PlyOptions &o)
{
    const PlyFlag *f = FindPlyFlag(flag);
    return f && f->read(value, o) ? std::string() : "bad value '" + value + "' of " + flag + ": " + (f ? f->expects : "no --ply-* flag with a value");
}

#endif  // APD_MI355X_HOST_PLY_OPTIONS_H_
