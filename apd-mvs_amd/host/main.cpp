// main.cpp -- drop-in driver of the PatchMatch path.
//
//   APD dense_folder [gpu_index | gpu,gpu,...] [--seed S] [--iters K] [--single-level] [--max-src N] [--keep-maps] [--no-fusion]
//       [--fusion eth|tat-intermediate|tat-advanced] [--files | --in-memory] [--jacobi] [--ranks N] [--no-rccl] [--rccl] [--masks [DIR]]
//       [--fusion-min-consistent N] [--fusion-reproj PX] [--fusion-depth REL] [--fusion-angle RAD] [--fusion-factors STRONG,WEAK]
//       [--ply-normals] [--ply-vis] [--ply-mean] [--ply-voxel SIZE] [--ply-stat-filter RADIUS,K,RATIO] [--ply-radius-filter RADIUS,MIN]
//       [--ply-component-filter RADIUS,MIN] [--ply-smooth RADIUS,MIN[,ITERATIONS]] [--ply-estimate-normals RADIUS,MIN]
//       [--ply-render-vis SPLAT,TOL] [--ply-register TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]]]
//       [--ply-align TRUTH.ply,RADIUS[,ITERATIONS[,scale]]] [--ply-align-planes TRUTH.ply,RADIUS[,ITERATIONS]]
//       [--ply-score TRUTH.ply,TAU] [--filtered-maps] [--mesh VOXEL[,TRUNC]] [--mesh-weld TOL] [--mesh-trim MIN_VIEWS[,MIN_PIXELS[,TOL]]] [--mesh-depth-maps] [--mesh-min-component FACES] [--mesh-smooth ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]]] [--mesh-simplify CELL[,mean|quadric]] [--mesh-normals] [--mesh-recolour [TOL[,MIN_COS]]] [--mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]]
//
// --mesh VOXEL[,TRUNC]: besides everything else, APD/APD.ply.mesh: a binary PLY with faces, the marching-tetrahedra mesh of a signed
// distance volume with samples VOXEL apart and a truncation distance of TRUNC (4 * VOXEL unless given) over the box of the points
// of APD.ply, integrated from the filtered maps of --filtered-maps (which need not be given) with the views' colours
// (apd_volume_create, apd_volume_integrate, apd_volume_extract_mesh; RunMesh, host/fusion.cpp).  Every driver takes it; refused
// with --no-fusion, which leaves no cloud to take the box from.  Without the flag no output changes.
// --mesh-weld TOL, --mesh-trim MIN_VIEWS[,MIN_PIXELS[,TOL]], --mesh-min-component FACES, --mesh-smooth
// ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]], --mesh-simplify CELL[,mean|quadric], --mesh-normals: what becomes of that mesh before it
// is written, in this fixed order whatever the order of the flags: vertices within TOL of each other, through chains, become the one with the smallest index and
// the faces that collapse go (apd_mesh_weld; VOXEL * 1e-4 welds only coincident vertices); the faces that fewer than MIN_VIEWS of
// the views see go with the vertices only they name -- a view sees a front face that owns MIN_PIXELS (1) pixels of the mesh rasterised
// into it or whose corners all lie within TOL (0.01) * depth behind that image (apd_mesh_remove_unseen, contract C25) --, before the
// component filter, which then removes what the trimming detached; the connected components of fewer than
// FACES faces go with the vertices only they name (apd_mesh_remove_small_components); every vertex moves ITERATIONS times towards the
// mean of its neighbours by LAMBDA (0.5) and then by MU (-0.53: Taubin's pair, which does not shrink; 0: plain Laplacian), the border
// vertices held (fixed), moved along the border (along, the default) or treated like the rest (free) (apd_mesh_smooth, contract C24);
// the vertices of one cell of size CELL become
// one, placed by the quadric of the faces around them or at their mean (apd_mesh_simplify, contract C23); the file carries nx ny
// nz, area-weighted vertex normals (apd_mesh_with_vertex_normals).  One line per step is printed with the counts before and after.  Each is refused
// without --mesh and on a malformed value, with the usage line, before anything is read.  Without them APD.ply.mesh keeps its bytes.
// --mesh-recolour [TOL[,MIN_COS]]: the last step, after --mesh-normals: every vertex takes its colour from the images of the views that
// see it through the final mesh's own z-buffer -- the four pixels around its projection within TOL (0.01) * depth of the rendered
// mesh, its normal at a cosine above MIN_COS (0.1, in [0, 1)) to the view (apd_mesh_colour_from_views, contract C26) -- and the volume
// is made without colour and integrated without the images: a third of its memory, the same geometry.  One line tells the vertices
// and how many no view coloured.  Needs --mesh; a malformed value gives the usage line before anything is read.
// --mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]: after everything else of --mesh, and changing no byte of APD.ply.mesh: the final mesh is
// scored against the vertices of the binary little-endian PLY file TRUTH.ply (apd_points_read_ply) at the threshold TAU
// (apd_mesh_score, contract C27): precision from DENSITY (4 / TAU^2) points per unit of area drawn on the surface under SEED (0), recall
// from every truth point's closest point of the surface.  One line in the format of --ply-score, and APD.ply.mesh.score.  Needs --mesh.
// --mesh-depth-maps: every view's depths_mesh.dmb beside depths_filtered.dmb, in the format of depths.dmb: the depth of the final
// mesh rasterised into the view, both sides drawn, 0 where it covers nothing (apd_mesh_render).  Needs --mesh.
//
// --filtered-maps: besides everything else, every view's depths_filtered.dmb, consistency.dmb (float, as depths.dmb) and votes.bin
// (bytes, as weak.bin) in <dense>/APD/<%08d>/: the geometric filter (apd_filter_views) on the final maps, with the --fusion-* rule
// (the defaults with a Tanks and Temples --fusion) and <dense>/blocks like the fusion.  Every driver takes it, with or without
// --no-fusion, and the files stay when the state files are removed.
//
// --fusion-*: the acceptance rule of the ETH fusion (apd_fusion_options, include/apd_mi355x.h: votes a point needs, the three
// thresholds, the STRONG / WEAK factors); refused with another --fusion, whose loops keep their own thresholds.  --ply-normals:
// APD.ply with nx ny nz, the reference pixel's normal, for every loop.  A bad value is refused with the usage line before
// anything is read or written.  Without these flags APD.ply keeps its bytes.  --ply-vis: APD/APD.ply.vis beside APD.ply, COLMAP's
// fused.ply.vis (per point the views that see it, as positions in pair.txt), from the same fusion; APD.ply keeps its bytes.
// --ply-mean: APD.ply holds every point's mean position over its own view and its agreeing sources (apd_points_average: what
// fusibile, ACMM and COLMAP emit) instead of the reference pixel's; with --ply-normals the mean normal, renormalised, too; with
// --ply-vis the lists of the averaged points.  With every --fusion.  A source contributes the pixel the point itself projects to;
// the Tanks and Temples loops may count a source through a stale `diff` entry of an earlier pixel, which that projection does not
// reach or finds without depth: such a source is skipped and no longer listed.  Without the flag nothing changes.
// --ply-voxel SIZE: APD.ply holds one point per occupied cell of a cubic grid of that cell size at the origin
// (apd_points_merge_voxels: the mean of the cell's points, the union of their lists) and, with --ply-vis, APD.ply.vis those
// lists; with --ply-mean the points are averaged first.  With every --fusion; the cells and the dropped points (non-finite, or
// 2^20 cells from the origin) are printed.  SIZE must be a positive finite number, or the usage line is all that happens.
// --ply-stat-filter RADIUS,K,RATIO: APD.ply holds the points whose mean distance to their K nearest neighbours within RADIUS is at
// most mu + RATIO * sigma of the cloud's own distribution of that value (apd_points_remove_statistical: the statistical outlier
// filter; a point with fewer than K neighbours within RADIUS goes) and, with --ply-vis, APD.ply.vis their lists; applied after
// --ply-mean and --ply-voxel and before --ply-radius-filter.  With every --fusion; the number removed and the threshold are
// printed.  RADIUS as for --ply-radius-filter, K 1 .. 64, RATIO a finite number (zero and negative allowed), or the usage line is
// all that happens.
// --ply-component-filter RADIUS,MIN: APD.ply holds the points whose connected component has at least MIN points
// (apd_points_remove_small_components: two points are joined when they are within RADIUS of each other, on the grid of cell size
// RADIUS at the origin; a detached clump goes whole, however dense it is) and, with --ply-vis, APD.ply.vis their lists; applied
// last, after --ply-radius-filter.  With every --fusion; the number of components and of removed points is printed.  RADIUS,MIN
// as for --ply-radius-filter, or the usage line is all that happens.
// --ply-smooth RADIUS,MIN[,ITERATIONS]: the points of APD.ply stand, where a point has at least MIN other points within RADIUS,
// on the weighted least-squares plane of that neighbourhood -- the weight of a neighbour at distance d is (1 - d^2 / RADIUS^2)^2 --
// ITERATIONS times (1 .. 16, 1 when left out), every point at once in each (apd_points_with_smoothed_positions, on the grid of
// cell size RADIUS at the origin): the depth noise along the viewing ray goes, a curved surface shrinks by up to RADIUS^2 / (2 R)
// per iteration.  Applied after --ply-component-filter and before --ply-estimate-normals and --ply-render-vis, which then act on
// the smoothed cloud.  With every --fusion; the number of points moved is printed; APD.ply.vis keeps its lists.  RADIUS,MIN as
// for --ply-estimate-normals, or the usage line is all that happens.
// --ply-estimate-normals RADIUS,MIN: the points of APD.ply carry, where a point has at least MIN other points within RADIUS, the
// normal of that neighbourhood -- its direction of least variance, signed like the point's own normal
// (apd_points_with_estimated_normals, on the grid of cell size RADIUS at the origin) -- instead of the reference pixel's or the mean
// one; applied after --ply-component-filter and --ply-smooth.  With every --fusion; the number of points estimated is printed.  The flag
// implies nothing else: the normals are in the file with --ply-normals, and without it APD.ply keeps its bytes.  RADIUS as for
// --ply-radius-filter, MIN a count of 2 or more, or the usage line is all that happens.
// --ply-render-vis SPLAT,TOL: APD.ply.vis (the flag implies --ply-vis) lists per point the views that see it, occlusion included:
// the cloud that APD.ply holds is drawn into every view's camera at the size of its image with a z-buffer, each point over the
// (2 SPLAT + 1)^2 pixels around its own, and a view sees a point that lies within TOL times the nearest depth behind that depth at
// its pixel (apd_points_rendered_visibility); applied last, after --ply-estimate-normals.  With every --fusion; APD.ply keeps the
// bytes it has without the flag, and the number of points no view sees is printed.  SPLAT must be a count of 0 .. 8 and TOL a
// non-negative finite number, or the usage line is all that happens.
// --ply-register TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]]: the points that APD.ply holds are moved onto the vertices of the binary
// little-endian PLY file TRUTH.ply from any start (apd_points_read_ply, apd_points_register: FPFH descriptors of the stored normals
// at RADIUS, their mutual matches, TRIALS (1 .. 65536, default 4096) RANSAC trials keyed by SEED (default 0) with inliers within
// DISTANCE, a refit; apd_points_transformed by its answer), after every other --ply-* flag but --ply-align and --ply-score, which
// then work on the moved points; TRUTH.ply is read once when several flags name it.  One line "Registered to ..." with every field
// of apd_points_registration_t is printed and APD.ply.register holds the same as one `name value` line per number, the doubles as
// %.17g.  APD.ply.vis keeps its bytes.  The value is read from its end: the longest tail of two to four numbers that fits.
// --ply-align TRUTH.ply,RADIUS[,ITERATIONS[,scale]]: the points that APD.ply holds are moved onto the vertices of the binary
// little-endian PLY file TRUTH.ply by point-to-point ICP within RADIUS (apd_points_read_ply, apd_points_align with ITERATIONS steps
// at most -- 1 .. 64, 16 without -- and the tolerance 1e-6, rigid, or a similarity with `scale`; apd_points_transformed by its
// answer).  Applied after every other --ply-* flag but --ply-score, which then scores the moved points; the file is read once
// when both name it.  APD.ply holds the moved positions and normals; APD.ply.vis keeps its bytes, since moving changes no list.
// One line "Aligned to ..." with every field of apd_points_alignment_t is printed -- rotation0 .. rotation8 row-major and
// translation0 .. translation2 -- and APD.ply.align holds the same as one `name value` line per number, the doubles as %.17g.
// The value is read from its end, since a file's name may hold commas; a bad one leaves the usage line as all that happens.
// --ply-align-planes TRUTH.ply,RADIUS[,ITERATIONS]: the points that APD.ply holds are moved onto the tangent planes of the
// vertices of the binary little-endian PLY file TRUTH.ply, which must hold nx ny nz, by point-to-plane ICP within RADIUS
// (apd_points_read_ply, apd_points_align_planes with ITERATIONS steps at most -- 1 .. 64, 16 without -- and the tolerance 1e-6;
// apd_points_transformed by its answer).  Applied after --ply-align, which brings the points within RADIUS first, and before
// --ply-score; TRUTH.ply is read once when several flags name it.  The normals of TRUTH.ply are used as stored and are not
// estimated here: a file without them has no usable match, and the line then shows stopped 2 and the identity.  One line "Aligned
// to planes of ..." with every field of apd_points_plane_alignment_t is printed and APD.ply.align_planes holds the same as one
// `name value` line per number, the doubles as %.17g.  APD.ply.vis keeps its bytes.  The value is read from its end.
// --ply-score TRUTH.ply,TAU: the points that APD.ply holds are scored against the vertices of the binary little-endian PLY file
// TRUTH.ply at the threshold TAU (apd_points_read_ply, apd_points_score, on the grid of cell size TAU at the origin): precision is
// the share of the points that have a vertex of TRUTH.ply within TAU, recall the share of those vertices that have a point within
// TAU, fscore their harmonic mean -- nearest-neighbour precision and recall at one threshold; --ply-align refines a registration
// first, but there is no initial global registration, no cropping volume and no occlusion-aware evaluation: to compare runs
// with each other.  Applied after every other --ply-* flag; APD.ply and APD.ply.vis
// keep the bytes they have without the flag.  One line with the nine fields of apd_points_score_t is printed, and APD.ply.score
// holds them as `key value` lines, the reals with 17 significant digits.  With every --fusion.  The value is split at its last
// comma; TAU as RADIUS of --ply-radius-filter, or the usage line is all that happens.  A file that cannot be read ends the run.
// --ply-radius-filter RADIUS,MIN: APD.ply holds the points that have at least MIN other points within RADIUS
// (apd_points_remove_sparse: the radius outlier filter, on the grid of cell size RADIUS at the origin) and, with --ply-vis,
// APD.ply.vis their lists; applied after --ply-mean, --ply-voxel and --ply-stat-filter.  With every --fusion; the number removed is printed.
// RADIUS must be a positive finite number whose square is one too, MIN a count, or the usage line is all that happens.
//
// --masks [DIR] (default DIR: masks): <dense_folder>/DIR/<%08d>.jpg|pgm are per-view pixel masks, grey < 128 = masked out of
// PatchMatch (apd_upload_mask: the pixels cost no NCC and leave as depth 0 / UNKNOWN); a view without a file is unmasked, a file
// of another size than its image is refused before anything is written.  Every driver takes it and writes the same bytes.
//
// One device index: the reference's driver.  A device LIST (or --jacobi): host/multi_device.cpp -- views sharded over the
// devices, state resident on them, depth maps all-gathered after every pass (RCCL when there is more than one rank -- its set-up takes seconds
// -- direct copies for a single rank; --rccl: RCCL even then; --no-rccl: direct copies only).  With --jacobi a single device runs
// one to three scheduler ranks, by frame size (--ranks N: exactly N).  --in-memory: the same scheduler with one rank in the
// reference's own order (a view of a geometric pass sees the depth maps its sources have at that moment): the bytes of the
// file-based driver without the files.
//
// Same command line, files and results as the reference driver (main.cpp:140-233), organised differently:
//   * pair.txt is read as one token stream with diagnostics (the reference never notices a missing or short file,
//     main.cpp:10);
//   * the passes are rows of one table (BuildSchedule) -- the same table apd-mvs_amd/pipeline.py::pass_schedule builds,
//     so the file-based and the in-memory scheduler cannot drift apart;
//   * every image is decoded once per process instead of once per (view, pass).
// --files: state moves between passes through depths.dmb / normals.dmb / weak.bin / selected_views.bin in <dense>/APD/<%08d>/,
// as in the reference; RunFusion then writes APD/APD.ply and the four state files are removed (--keep-maps keeps them).
// Default for one device: the same order of views and the same bytes with the state resident on the device (host/multi_device.cpp,
// --in-memory) when the folder fits it -- the files of the last pass are written with --keep-maps.
// Not built: the debug JPEGs of show_medium_result.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "APD.h"
#include "schedule.h"

namespace {

bool ParseOptions(int argc, char **argv, Options &o)
{
    if (argc < 2) {
        return false;
    }
    o.dense_folder = path(argv[1]);
    std::string mesh_flag;   // the last --mesh-* flag seen: each needs --mesh
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        auto value = [&](uint64_t &dst) {
            if (i + 1 >= argc) {
                return false;
            }
            dst = strtoull(argv[++i], nullptr, 10);
            return true;
        };
        const auto real = ply_value::Real;   // a non-negative finite number that fills the whole token
        auto threshold = [&](float &dst) {
            const char *text = i + 1 < argc ? argv[++i] : "";
            if (!real(text, dst)) {
                fprintf(stderr, "bad value '%s' of %s: a non-negative number\n", text, a.c_str());
                return false;
            }
            o.fusion_thresholds_set = true;
            return true;
        };
        uint64_t v = 0;
        if (a == "--fusion-min-consistent") {
            const char *text = i + 1 < argc ? argv[++i] : "";
            char *end = nullptr;
            const long n = strtol(text, &end, 10);
            if (end == text || *end != '\0' || n < 1 || n > APD_MAX_IMAGES) {
                fprintf(stderr, "bad value '%s' of %s: 1 .. %d\n", text, a.c_str(), APD_MAX_IMAGES);
                return false;
            }
            o.fusion.min_consistent = (int)n;
            o.fusion_thresholds_set = true;
        } else if (a == "--fusion-reproj") {
            if (!threshold(o.fusion.max_reproj_error)) return false;
        } else if (a == "--fusion-depth") {
            if (!threshold(o.fusion.max_relative_depth)) return false;
        } else if (a == "--fusion-angle") {
            if (!threshold(o.fusion.max_angle)) return false;
        } else if (a == "--fusion-factors") {
            const std::string both = i + 1 < argc ? argv[++i] : "";
            const size_t comma = both.find(',');
            if (comma == std::string::npos || !real(both.substr(0, comma).c_str(), o.fusion.factor_strong) ||
                !real(both.substr(comma + 1).c_str(), o.fusion.factor_weak)) {
                fprintf(stderr, "bad value '%s' of %s: STRONG,WEAK, two non-negative numbers\n", both.c_str(), a.c_str());
                return false;
            }
            o.fusion_thresholds_set = true;
        } else if (a == "--ply-normals") {
            o.fusion.ply_normals = 1;
        } else if (a == "--ply-vis") {
            o.ply.vis = true;
        } else if (a == "--ply-mean") {
            o.ply.mean = true;
        } else if (FindPlyFlag(a)) {   // every --ply-* flag with a value (host/ply_options.h)
            const std::string why = ParsePlyOption(a, i + 1 < argc ? argv[++i] : "", o.ply);
            if (!why.empty()) {
                fprintf(stderr, "%s\n", why.c_str());
                return false;
            }
        } else if (a == "--filtered-maps") {
            o.filtered_maps = true;
        } else if (a == "--mesh") {
            const std::string both = i + 1 < argc ? argv[++i] : "";
            const std::vector<std::string> t = ply_value::Split(both, 1);
            float voxel = 0.0f, trunc = 0.0f;
            if (!ply_value::Radius(t.empty() ? both : t[0], voxel) || (!t.empty() && !ply_value::Radius(t[1], trunc))) {
                fprintf(stderr, "bad value '%s' of %s: VOXEL[,TRUNC], positive numbers\n", both.c_str(), a.c_str());
                return false;
            }
            o.mesh_voxel = voxel;
            o.mesh_trunc = t.empty() ? 4.0f * voxel : trunc;
        } else if (a == "--mesh-weld") {
            const std::string text = i + 1 < argc ? argv[++i] : "";
            if (!ply_value::Radius(text, o.mesh_clean.weld)) {
                fprintf(stderr, "bad value '%s' of %s: TOL, a positive number\n", text.c_str(), a.c_str());
                return false;
            }
            mesh_flag = a;
        } else if (a == "--mesh-trim") {
            const std::string all = i + 1 < argc ? argv[++i] : "";
            std::vector<std::string> t;
            for (size_t from = 0; t.size() < 4; ) {
                const size_t comma = all.find(',', from);
                t.push_back(all.substr(from, comma == std::string::npos ? std::string::npos : comma - from));
                if (comma == std::string::npos) {
                    break;
                }
                from = comma + 1;
            }
            MeshClean c = o.mesh_clean;
            unsigned long long views = 0, pixels = 1;
            bool good = t.size() <= 3 && ply_value::Count(t[0], 1, 0x7fffffffull, views);
            if (good && t.size() > 1) {
                good = ply_value::Count(t[1], 1, 0x7fffffffull, pixels);
            }
            if (good && t.size() > 2) {
                char *end = nullptr;
                c.trim_tolerance = strtof(t[2].c_str(), &end);
                good = end != t[2].c_str() && *end == '\0' && std::isfinite(c.trim_tolerance) && c.trim_tolerance >= 0.0f;
            }
            if (!good) {
                fprintf(stderr, "bad value '%s' of %s: MIN_VIEWS[,MIN_PIXELS[,TOL]], counts of at least 1 and a number that is not negative\n", all.c_str(),
                        a.c_str());
                return false;
            }
            c.trim = (unsigned)views;
            c.trim_pixels = (unsigned)pixels;
            o.mesh_clean = c;
            mesh_flag = a;
        } else if (a == "--mesh-depth-maps") {
            o.mesh_clean.depth_maps = true;
        } else if (a == "--mesh-min-component") {
            const std::string text = i + 1 < argc ? argv[++i] : "";
            unsigned long long n = 0;
            if (!ply_value::Count(text, 0, 0x7fffffffull, n)) {
                fprintf(stderr, "bad value '%s' of %s: FACES, a count\n", text.c_str(), a.c_str());
                return false;
            }
            o.mesh_clean.remove_small = true;
            o.mesh_clean.min_component = (unsigned)n;
            mesh_flag = a;
        } else if (a == "--mesh-smooth") {
            const std::string all = i + 1 < argc ? argv[++i] : "";
            std::vector<std::string> t;
            for (size_t from = 0; t.size() < 5; ) {
                const size_t comma = all.find(',', from);
                t.push_back(all.substr(from, comma == std::string::npos ? std::string::npos : comma - from));
                if (comma == std::string::npos) {
                    break;
                }
                from = comma + 1;
            }
            MeshClean c = o.mesh_clean;
            unsigned long long n = 0;
            char *end = nullptr;
            bool good = t.size() <= 4 && ply_value::Count(t[0], 1, 1000, n);
            if (good && t.size() > 1) {
                good = ply_value::Real(t[1], c.smooth_lambda) && c.smooth_lambda > 0.0f && c.smooth_lambda <= 1.0f;
            }
            if (good && t.size() > 2) {
                c.smooth_mu = strtof(t[2].c_str(), &end);
                good = end != t[2].c_str() && *end == '\0' && c.smooth_mu >= -2.0f && c.smooth_mu <= 0.0f;
            }
            if (good && t.size() > 3) {
                c.smooth_boundary = t[3] == "fixed" ? APD_SMOOTH_BOUNDARY_FIXED : t[3] == "along" ? APD_SMOOTH_BOUNDARY_ALONG : t[3] == "free" ? APD_SMOOTH_BOUNDARY_FREE : -1;
                good = c.smooth_boundary >= 0;
            }
            if (!good) {
                fprintf(stderr, "bad value '%s' of %s: ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]], a count of 1 .. 1000, LAMBDA in (0, 1], MU in [-2, 0]\n", all.c_str(),
                        a.c_str());
                return false;
            }
            c.smooth = (int)n;
            o.mesh_clean = c;
            mesh_flag = a;
        } else if (a == "--mesh-simplify") {
            const std::string both = i + 1 < argc ? argv[++i] : "";
            const size_t comma = both.find(',');
            const std::string how = comma == std::string::npos ? "quadric" : both.substr(comma + 1);
            if (!ply_value::Radius(both.substr(0, comma), o.mesh_clean.simplify) || (how != "mean" && how != "quadric")) {
                o.mesh_clean.simplify = 0.0f;
                fprintf(stderr, "bad value '%s' of %s: CELL[,mean|quadric], CELL a positive number\n", both.c_str(), a.c_str());
                return false;
            }
            o.mesh_clean.simplify_mean = how == "mean";
            mesh_flag = a;
        } else if (a == "--mesh-normals") {
            o.mesh_clean.normals = true;
            mesh_flag = a;
        } else if (a == "--mesh-recolour") {
            MeshClean c = o.mesh_clean;
            if (i + 1 < argc && argv[i + 1][0] != '-') {   // the value is optional
                const std::string both = argv[++i];
                const size_t comma = both.find(',');
                bool good = ply_value::Real(both.substr(0, comma), c.recolour_tolerance) && c.recolour_tolerance >= 0.0f;
                if (good && comma != std::string::npos) {
                    good = ply_value::Real(both.substr(comma + 1), c.recolour_min_cos) && c.recolour_min_cos >= 0.0f && c.recolour_min_cos < 1.0f;
                }
                if (!good) {
                    fprintf(stderr, "bad value '%s' of %s: [TOL[,MIN_COS]], a number that is not negative and one in [0, 1)\n", both.c_str(), a.c_str());
                    return false;
                }
            }
            c.recolour = true;
            o.mesh_clean = c;
            mesh_flag = a;
        } else if (a == "--mesh-score") {
            const std::string all = i + 1 < argc ? argv[++i] : "";
            MeshClean c = o.mesh_clean;
            bool good = false;
            for (size_t cuts = 3; cuts >= 1 && !good; --cuts) {   // the file's name may hold commas: the most trailing numbers that parse
                const std::vector<std::string> t = ply_value::Split(all, cuts, true);
                unsigned long long seed = 0;
                float density = 0.0f;
                good = !t.empty() && ply_value::Radius(t[1], c.score_threshold) && (cuts < 2 || (ply_value::Real(t[2], density) && density > 0.0f)) &&
                       (cuts < 3 || ply_value::Count(t[3], 0, ~0ull, seed));
                if (good) {
                    c.score_truth = t[0];
                    c.score_density = cuts < 2 ? 0.0 : strtod(t[2].c_str(), nullptr);
                    c.score_seed = seed;
                }
            }
            if (!good) {
                fprintf(stderr, "bad value '%s' of %s: TRUTH.ply,TAU[,DENSITY[,SEED]], a file, a positive number, a positive number and an integer\n", all.c_str(),
                        a.c_str());
                return false;
            }
            o.mesh_clean = c;
            mesh_flag = a;
        } else if (a == "--seed") {
            if (!value(o.seed)) return false;
        } else if (a == "--iters") {
            if (!value(v)) return false;
            o.iters = (int)v;
        } else if (a == "--max-src") {
            if (!value(v)) return false;
            o.max_src = (int)v;
        } else if (a == "--single-level") {
            o.single_level = true;
        } else if (a == "--keep-maps") {
            o.keep_maps = true;
        } else if (a == "--no-fusion") {
            o.no_fusion = true;
        } else if (a == "--fusion") {
            const std::string name = i + 1 < argc ? argv[++i] : "";
            if (name == "eth") {
                o.fusion_variant = APD_FUSION_ETH;
            } else if (name == "tat-intermediate") {
                o.fusion_variant = APD_FUSION_TAT_INTERMEDIATE;
            } else if (name == "tat-advanced") {
                o.fusion_variant = APD_FUSION_TAT_ADVANCED;
            } else {
                fprintf(stderr, "bad fusion '%s': eth, tat-intermediate or tat-advanced\n", name.c_str());
                return false;
            }
        } else if (a == "--masks") {
            o.masks_dir = (i + 1 < argc && argv[i + 1][0] != '-') ? argv[++i] : "masks";
            if (o.masks_dir.empty()) {
                return false;
            }
        } else if (a == "--late-fusion-inputs") {
            o.late_fusion_inputs = true;
        } else if (a == "--scheduler-free-gb" && i + 1 < argc) {
            o.scheduler_free_gb = atof(argv[++i]);
        } else if (a == "--clean-exit") {
            o.clean_exit = true;
        } else if (a == "--copy-images") {
            o.copy_images = true;
        } else if (a == "--jacobi") {
            o.jacobi = true;
        } else if (a == "--in-memory") {
            o.in_memory = true;
        } else if (a == "--files") {
            o.files = true;
        } else if (a == "--ranks") {
            if (!value(v)) return false;
            o.ranks_per_device = (int)v;
        } else if (a == "--no-rccl") {
            o.use_rccl = false;
        } else if (a == "--exchange-device-sync") {
            o.exchange_device_sync = true;
        } else if (a == "--rccl") {
            o.force_rccl = true;
        } else if (i == 2 && a.size() && a[0] != '-') {
            // positional, as in the reference (main.cpp:149-153); additive: a comma-separated list = one scheduler rank per entry
            o.devices.clear();
            size_t pos = 0;
            while (pos <= a.size()) {
                const size_t comma = a.find(',', pos);
                const std::string item = a.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
                char *end = nullptr;
                const long d = strtol(item.c_str(), &end, 10);
                if (item.empty() || *end != '\0') {
                    fprintf(stderr, "bad device list '%s'\n", a.c_str());
                    return false;
                }
                o.devices.push_back((int)d);
                if (comma == std::string::npos) {
                    break;
                }
                pos = comma + 1;
            }
            o.gpu_index = o.devices[0];
        } else {
            fprintf(stderr, "unknown argument '%s'\n", a.c_str());
            return false;
        }
    }
    if (o.fusion_thresholds_set && o.fusion_variant != APD_FUSION_ETH) {
        fprintf(stderr, "--fusion-min-consistent, --fusion-reproj, --fusion-depth, --fusion-angle and --fusion-factors apply to --fusion eth only\n");
        return false;
    }
    if (o.mesh_clean.depth_maps && !(o.mesh_voxel > 0.0f)) {
        fprintf(stderr, "--mesh-depth-maps renders the mesh of --mesh VOXEL[,TRUNC]: not without it\n");
        return false;
    }
    if (!mesh_flag.empty() && !(o.mesh_voxel > 0.0f)) {
        fprintf(stderr, "%s changes the mesh of --mesh VOXEL[,TRUNC]: not without it\n", mesh_flag.c_str());
        return false;
    }
    if (o.mesh_voxel > 0.0f && o.no_fusion) {
        fprintf(stderr, "--mesh takes its box from the fused points: not with --no-fusion\n");
        return false;
    }
    o.fusion.variant = o.fusion_variant;
    return true;
}

// pair.txt (written by colmap2mvsnet.py:449-456): <num views>, then per view <ref id> and <n> followed by n
// (<source id> <score>) pairs.  Sources with score <= 0 are not used (main.cpp:43).  Returns an empty string or what is
// wrong with the file.
std::string ReadPairFile(const path &file, const path &dense_folder, std::vector<Problem> &problems)
{
    problems.clear();
    std::ifstream in(file);
    if (!in) {
        return "cannot open " + file.string();
    }
    const std::vector<std::string> tok{std::istream_iterator<std::string>(in), std::istream_iterator<std::string>()};
    size_t at = 0;
    auto number = [&](double &out) {
        if (at >= tok.size()) {
            return false;
        }
        char *end = nullptr;
        out = strtod(tok[at].c_str(), &end);
        const bool ok = end != tok[at].c_str() && *end == '\0';
        ++at;
        return ok;
    };
    double count = 0;
    if (!number(count) || count < 0) {
        return file.string() + ": no view count";
    }
    for (int i = 0; i < (int)count; ++i) {
        double id = 0, n = 0;
        if (!number(id) || !number(n) || n < 0) {
            return file.string() + ": entry " + std::to_string(i) + " is incomplete (token " + std::to_string(at) + ")";
        }
        Problem p;
        p.index = i;
        p.ref_image_id = (int)id;
        p.dense_folder = dense_folder;
        p.result_folder = dense_folder / "APD" / ToFormatIndex(p.ref_image_id);
        for (int j = 0; j < (int)n; ++j) {
            double src = 0, score = 0;
            if (!number(src) || !number(score)) {
                return file.string() + ": view " + std::to_string(p.ref_image_id) + " lists " + std::to_string((int)n) +
                       " sources but holds fewer";
            }
            if ((float)score > 0.0f) {
                p.src_image_ids.push_back((int)src);
            }
        }
        problems.push_back(std::move(p));
    }
    return std::string();
}

// main.cpp:51-70: every reference image must exist and have the size of the first one.  The sizes of the source images
// and of the prior maps are checked where they are loaded (APD::InuputInitialization).
bool CheckImages(const std::vector<Problem> &problems, int &width, int &height)
{
    width = height = 0;
    for (const Problem &p : problems) {
        Mat image;
        if (!ReadGrayImageShared(p.dense_folder / "images" / ToFormatIndex(p.ref_image_id), image)) {
            return false;
        }
        if (width == 0) {
            width = image.cols;
            height = image.rows;
        } else if (image.cols != width || image.rows != height) {
            return false;
        }
    }
    return !problems.empty();
}

}  // namespace

// One (view, pass): the reference's ProcessProblem (main.cpp:91-138) -- run the path, post-process (depth outside the
// search range -> 0 and UNKNOWN, main.cpp:109-112), write the four state files.
void ProcessProblem(const Problem &problem)
{
    printf("Processing image: %08d...\n", problem.ref_image_id);
    const auto t0 = std::chrono::steady_clock::now();
    APD apd(problem);
    apd.InuputInitialization();
    apd.CudaSpaceInitialization();
    apd.SetDataPassHelperInCuda();
    apd.RunPatchMatch();
    const int W = apd.GetWidth(), H = apd.GetHeight();
    const float lo = apd.GetDepthMin(), hi = apd.GetDepthMax();
    Mat depth(H, W, MAT_32FC1), normal(H, W, MAT_32FC3), states = apd.GetPixelStates();
    ParallelFor((size_t)H, [&](size_t row) {
        float *d = depth.ptr<float>((int)row);
        Vec3f *n = normal.ptr<Vec3f>((int)row);
        uint8_t *s = states.ptr<uint8_t>((int)row);
        for (int c = 0; c < W; ++c) {
            const float4 h = apd.GetPlaneHypothesis((int)row, c);
            const bool out_of_range = h.w < lo || h.w > hi;  // false for NaN, as in the reference
            d[c] = out_of_range ? 0.0f : h.w;
            if (out_of_range) {
                s[c] = UNKNOWN;
            }
            n[c] = Vec3f{{h.x, h.y, h.z}};
        }
    });
    const std::string unwritten = WriteStateFiles(problem.result_folder, depth, normal, states, apd.GetSelectedViews());
    if (!unwritten.empty()) {
        fprintf(stderr, "cannot write %s\n", unwritten.c_str());
        exit(EXIT_FAILURE);
    }
    const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    printf("Processing image: %08d done!\nCost time: %lld ms\n", problem.ref_image_id, (long long)ms);
    fflush(stdout);
}

int main(int argc, char **argv)
{
    const auto t_start = std::chrono::steady_clock::now();
    // Views in flight run on their own HIP streams, and the runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4):
    // two streams that land on one queue take turns.  Eight queues: 24 x 1080p passes 7.70 -> 7.58 s with six views in flight, and the
    // 1.3 s round 5 charged to the peer-copy exchange of `0,0 --no-rccl` (8.82 -> 7.54 s: its two lanes shared a queue; loading librccl
    // happened to shift the mapping) -- profiles/r06/ab_hw_queues.txt.  Read by the HIP runtime when it starts, i.e. at the first HIP
    // call below; a value the caller has set is kept.
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    Options opt;
    if (!ParseOptions(argc, argv, opt)) {
        fprintf(stderr, "USAGE: APD dense_folder [gpu_index | gpu,gpu,...] [--seed S] [--iters K] [--single-level] [--max-src N] [--keep-maps] [--no-fusion] [--fusion eth|tat-intermediate|tat-advanced] [--fusion-min-consistent N] [--fusion-reproj PX] [--fusion-depth REL] [--fusion-angle RAD] [--fusion-factors STRONG,WEAK] [--ply-normals] [--ply-vis] [--ply-mean] [--ply-voxel SIZE] [--ply-stat-filter RADIUS,K,RATIO] [--ply-radius-filter RADIUS,MIN] [--ply-component-filter RADIUS,MIN] [--ply-smooth RADIUS,MIN[,ITERATIONS]] [--ply-estimate-normals RADIUS,MIN] [--ply-render-vis SPLAT,TOL] [--ply-register TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]]] [--ply-align TRUTH.ply,RADIUS[,ITERATIONS[,scale]]] [--ply-align-planes TRUTH.ply,RADIUS[,ITERATIONS]] [--ply-score TRUTH.ply,TAU] [--filtered-maps] [--mesh VOXEL[,TRUNC]] [--mesh-weld TOL] [--mesh-trim MIN_VIEWS[,MIN_PIXELS[,TOL]]] [--mesh-depth-maps] [--mesh-min-component FACES] [--mesh-smooth ITERATIONS[,LAMBDA[,MU[,fixed|along|free]]]] [--mesh-simplify CELL[,mean|quadric]] [--mesh-normals] [--mesh-recolour [TOL[,MIN_COS]]] [--mesh-score TRUTH.ply,TAU[,DENSITY[,SEED]]] [--files | --in-memory] [--jacobi] [--ranks N] [--no-rccl] [--rccl] [--masks [DIR]] [--exchange-device-sync] [--late-fusion-inputs] [--copy-images] [--clean-exit]\n"
                        "  --ply-mean: APD.ply with every point's mean position (--ply-normals: and normal) over the views that agree on it; with every --fusion.\n"
                        "      A source that a Tanks and Temples loop counted through a stale entry and the point's own projection does not reach is skipped.\n"
                        "  --ply-voxel SIZE: APD.ply (and APD.ply.vis) with one point per cell of a cubic grid of cell size SIZE, after --ply-mean if both are given.\n"
                        "  --ply-stat-filter RADIUS,K,RATIO: APD.ply (and APD.ply.vis) without the points whose mean distance to their K nearest neighbours within RADIUS is above mean + RATIO * deviation of the cloud's, after --ply-mean and --ply-voxel, before --ply-radius-filter.\n"
                        "  --ply-radius-filter RADIUS,MIN: APD.ply (and APD.ply.vis) without the points that have fewer than MIN other points within RADIUS, after --ply-mean and --ply-voxel.\n"
                        "  --ply-component-filter RADIUS,MIN: APD.ply (and APD.ply.vis) without the points of connected components of fewer than MIN points, two points being joined when they are within RADIUS of each other, after --ply-radius-filter.\n"
                        "  --ply-smooth RADIUS,MIN[,ITERATIONS]: the points of APD.ply (and of what --ply-estimate-normals and --ply-render-vis then see) each projected on the weighted plane of the other points within RADIUS of it, where there are at least MIN (2 or more) of them, ITERATIONS (1 .. 16, default 1) times, after --ply-component-filter.\n"
                        "  --ply-estimate-normals RADIUS,MIN: the normals of the points of APD.ply (shown with --ply-normals) estimated from the other points within RADIUS of each, where there are at least MIN (2 or more) of them, after every other --ply-* flag but --ply-render-vis.\n"
                        "  --ply-render-vis SPLAT,TOL: APD.ply.vis (implies --ply-vis) lists per point the views that see it when the points of APD.ply are drawn into every view with a z-buffer, each over the (2 SPLAT + 1)^2 pixels around its own (SPLAT 0 .. 8), within TOL times the nearest depth at its pixel; after every other --ply-* flag but --ply-register, --ply-align and --ply-score.\n"
                        "  --ply-register TRUTH.ply,RADIUS,DISTANCE[,TRIALS[,SEED]]: the points of APD.ply are moved onto the vertices of the binary PLY file TRUTH.ply from any start, at a scale that is about right: FPFH descriptors of the stored normals at RADIUS, their mutual matches, TRIALS (1 .. 65536, default 4096) RANSAC trials keyed by SEED (default 0) with inliers within DISTANCE, a refit; prints the transform and writes it to APD.ply.register; after every other --ply-* flag but --ply-align and --ply-score, which work on the moved points; APD.ply.vis is unchanged.\n"
                        "  --ply-align TRUTH.ply,RADIUS[,ITERATIONS[,scale]]: the points of APD.ply are moved onto the vertices of the binary PLY file TRUTH.ply by point-to-point ICP within RADIUS, at most ITERATIONS (1 .. 64, default 16) steps, rigid or with `scale` a similarity; prints the transform and writes it to APD.ply.align; after every other --ply-* flag but --ply-score, APD.ply.vis is unchanged.\n"
                        "  --ply-align-planes TRUTH.ply,RADIUS[,ITERATIONS]: the points of APD.ply are moved onto the tangent planes of the vertices of the binary PLY file TRUTH.ply, which needs nx ny nz (its normals are used as stored, not estimated), by point-to-plane ICP within RADIUS, at most ITERATIONS (1 .. 64, default 16) steps, rigid; prints the transform and writes it to APD.ply.align_planes; after --ply-align and before --ply-score, APD.ply.vis is unchanged.\n"
                        "  --ply-score TRUTH.ply,TAU: prints, and writes to APD.ply.score, the precision, recall and F-score of the points of APD.ply against the vertices of the binary PLY file TRUTH.ply at the threshold TAU: the share of each cloud that has a point of the other within TAU; after every other --ply-* flag, --ply-align included (it then scores the aligned points, and TRUTH.ply is read once when both name it), APD.ply keeps its bytes.\n");
        return EXIT_FAILURE;
    }
    if (opt.devices.empty()) {
        opt.devices.push_back(opt.gpu_index);
    }
    for (int d : opt.devices) {
        if (d < 0 || d >= apd_device_count()) {
            fprintf(stderr, "Requested GPU %d, found %d device(s)\n", d, apd_device_count());
            return EXIT_FAILURE;
        }
    }
    APD::SetDevice(opt.gpu_index);
    SetFusionDevice(opt.gpu_index);
    SetFusionOptions(opt.fusion);
    SetFusionPly(opt.ply);

    std::vector<Problem> problems;
    const std::string why = ReadPairFile(opt.dense_folder / "pair.txt", opt.dense_folder, problems);
    if (!why.empty()) {
        fprintf(stderr, "%s\n", why.c_str());
        return EXIT_FAILURE;
    }
    if (!opt.masks_dir.empty()) {   // every mask file against its image, before a result folder exists
        for (Problem &p : problems) {
            p.masks_dir = opt.masks_dir;
            Mat mask;
            if (ReadViewMask(opt.dense_folder, opt.masks_dir, p.ref_image_id, mask) < 0) {
                return EXIT_FAILURE;
            }
        }
    }
    std::vector<int> ids;  // every image any pass will read
    for (Problem &p : problems) {
        if (opt.max_src > 0 && (int)p.src_image_ids.size() > opt.max_src) {
            p.src_image_ids.resize((size_t)opt.max_src);
        }
        std::filesystem::create_directories(p.result_folder);
        ids.push_back(p.ref_image_id);
        ids.insert(ids.end(), p.src_image_ids.begin(), p.src_image_ids.end());
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    // Sources without an entry of their own (a subset of the views is reconstructed) are loaded like any other image
    // (APD.cpp:419-452): they contribute no depth map to the geometric term and take no part in the fusion (host/APD.cpp,
    // host/fusion.cpp; apd-mvs_amd/pipeline.py does the same).  A view that lists itself is refused: the fusion would count it
    // as its own witness.
    for (const Problem &p : problems) {
        for (int s : p.src_image_ids) {
            if (s == p.ref_image_id) {
                fprintf(stderr, "pair.txt: view %d lists itself as a source\n", s);
                return EXIT_FAILURE;
            }
        }
    }
    {
        std::vector<int> refs;
        for (const Problem &p : problems) {
            refs.push_back(p.ref_image_id);
        }
        APD::SetReconstructedViews(refs);
    }
    PrefetchGrayImages(opt.dense_folder / "images", ids);  // decoded once, on several host threads
    if (opt.files && (opt.in_memory || opt.jacobi || opt.devices.size() > 1)) {
        fprintf(stderr, "--files is the single-device driver (no device list, --jacobi or --in-memory)\n");
        return EXIT_FAILURE;
    }
    // `APD dense_folder [gpu]`, the reference's command line: its order of views and its bytes, in memory when the folder fits the
    // device (InMemoryBytesPerPixel: level images, two sets of depth maps, every view's state, the handles of the views in flight, the
    // final maps and the fusion's buffers), through the files otherwise or with --files.
    bool auto_in_memory = false;   // the in-memory scheduler was this function's choice, not the command line's
    if (!opt.files && !opt.in_memory && !opt.jacobi && opt.devices.size() == 1) {
        int w = 0, h = 0;
        if (CheckImages(problems, w, h)) {
            size_t max_src = 1;
            for (const Problem &p : problems) {
                max_src = std::max(max_src, p.src_image_ids.size());
            }
            // the scheduler's own test (same function, same free-memory figure and --scheduler-free-gb cap), BEFORE it loads a single
            // full-size image or prints its header: a folder that does not fit goes to the file loop at once
            const int lanes = InMemoryLanes(opt, w, h, (int)problems.size(), 1, true);   // the count RunMultiDevice will use
            const InMemoryFit fit = TestInMemoryFit(opt, opt.gpu_index, w, h, (int)ids.size(), (int)problems.size(), 1, lanes, (int)max_src);
            opt.in_memory = fit.have_memory && fit.fits;
            auto_in_memory = opt.in_memory;
            if (fit.have_memory && !fit.fits) {
                printf("%.1f GB of resident state against %.1f GB free on device %d: this folder does not fit the in-memory scheduler, passing state through files\n",
                       fit.need_bytes / 1e9, fit.free_bytes / 1e9, opt.gpu_index);
            }
        }
    }
    if (opt.in_memory && (opt.devices.size() > 1 || opt.jacobi)) {
        fprintf(stderr, "--in-memory keeps the reference's order of views: one device, one rank (no device list, no --jacobi)\n");
        return EXIT_FAILURE;
    }
    if (opt.devices.size() > 1 || opt.jacobi || opt.in_memory) {
        printf("Start-up (pair.txt, image decode on several threads, device query): %lld ms\n",
               (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_start).count());
        const int rc = RunMultiDevice(opt, problems);  // host/multi_device.cpp: in memory, views sharded over the device list
        if (rc == kExitDoesNotFit && auto_in_memory) {
            // the plain `APD folder gpu` command line must process every folder the file driver can (free memory may have shrunk
            // between the estimate above and the scheduler's own): nothing has been run or written yet, take the files
            printf("in-memory scheduler refused the folder: passing state through files\n");
            opt.in_memory = false;
        } else {
            // Every file is written and closed.  Leaving through _Exit skips the one-by-one release of tens of gigabytes of device memory
            // and the runtime's own teardown (half a second at 152 views): the driver reclaims a process's memory in one step.
            // (--clean-exit returns normally: a profiler that writes its output from an exit handler -- rocprofv3 -- needs that.)
            const int code = rc == kExitDoesNotFit ? EXIT_FAILURE : rc;
            fflush(stdout);
            fflush(stderr);
            if (!opt.clean_exit) {
                std::_Exit(code);
            }
            return code;
        }
    }
    int width = 0, height = 0;
    if (!CheckImages(problems, width, height)) {
        fprintf(stderr, "Images may error, check it!\n");  // the reference's message (main.cpp:158)
        return EXIT_FAILURE;
    }
    printf("There are %zu problems needed to be processed!\n", problems.size());
    const int round_num = opt.single_level ? 1 : RoundNum(width, height);
    printf("Round nums: %d\n", round_num);

    for (const Pass &pass : BuildSchedule(round_num, opt.single_level)) {
        for (Problem &p : problems) {
            Configure(p, pass, opt);
            ProcessProblem(p);
        }
        if (pass.iteration % 4 == 3) {
            printf("Round: %d done\n", pass.level);
        }
    }
    if (opt.filtered_maps) {
        RunFilter(opt.dense_folder, problems);
    }
    if (!opt.no_fusion) {
        RunFusion(opt.dense_folder, problems);  // main.cpp:219
        if (opt.mesh_voxel > 0.0f) {
            RunMesh(opt.dense_folder, problems, opt.mesh_voxel, opt.mesh_trunc, opt.mesh_clean);
        }
        if (!opt.keep_maps) {                   // main.cpp:220-230
            for (const Problem &p : problems) {
                for (const char *name : kStateFiles) {
                    std::filesystem::remove(p.result_folder / name);
                }
            }
        }
    }
    printf("All done\n");
    return EXIT_SUCCESS;
}
