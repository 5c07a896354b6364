// apd_mesh_math.h -- what cleaning an indexed triangle mesh computes (arithmetic contract C22): the rules under
// apd_mesh_weld, apd_mesh_components / apd_mesh_remove_small_components and apd_mesh_with_vertex_normals, written once and compiled
// by hipcc into the kernels (apd_mesh.hip) and by the host compiler into the sequential checker (tests/helpers/mesh_ref.cpp).  As in
// apd_volume_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order.
//
// A mesh: V vertices (position, 3 x binary32; optionally colour, 3 bytes; optionally normal, 3 x binary32) and F faces of three
// indices in [0, V).  A face may repeat an index.  Every operation leaves its input as it is and its result is a function of the
// input alone.
//
// Weld(tolerance, origin).  The graph of contract C13 over the vertex positions with radius = tolerance: an edge between two
// vertices that are neighbours by contract C11 (apd_radius_math.h) on the grid of cell size `tolerance` at `origin`; a vertex outside
// the grid (a non-finite coordinate, a cell beyond +-2^20) has no edge.  rep[v] = the smallest index of v's component.  Every face
// index i becomes rep[i]; a face with two equal indices after that is dropped (mesh_face_degenerate); a vertex survives when
// rep[v] == v and a surviving face names it; surviving vertices and faces keep their input order and the faces are renumbered.  A
// representative keeps its own position, colour and normal: nothing is averaged.  -0.0 and +0.0 are at distance 0.
//
// Components.  Two faces are adjacent when they name a common vertex index; a component is the closure.  label[f] = the smallest
// face index of f's component, size[f] = its number of faces.  Removal(min_faces) keeps the faces with size[f] >= min_faces in input
// order -- 0 and 1 keep every face --, drops the vertices that no kept face names and renumbers.
//
// Vertex normals, area-weighted.  Face f with corners a, b, c at positions widened to binary64 (exact): u = b - a, w = c - a per
// component, g = (u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x): every product and every difference one
// binary64 operation (mesh_face_normal).  s_v = the sum of g over the corners (f, c) with index[3 f + c] == v, in ascending 3 f + c,
// in binary64, from +0.0 (mesh_add).  len = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z); n = (float)(s / len) per component when len
// is finite and > 0.0, else (0, 0, 0) (mesh_vertex_normal).  A vertex no face names gets zeros; a face that repeats an index adds
// its g, which is exactly zero when the repeated corner is a (u or w is zero) or b == c (the products cancel) and is a NaN only
// where a position is not finite.  binary64 sqrt and division are correctly rounded on both sides, as contract C18 relies on.
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_radius_math.h"

namespace apd_fusion {

// A face that names a vertex twice: what welding drops
APD_HD bool mesh_face_degenerate(int32_t a, int32_t b, int32_t c) { return a == b || a == c || b == c; }

// g: the cross product (B - A) x (C - A) in binary64, twice the face's area along its right-hand normal
APD_HD void mesh_face_normal(const float A[3], const float B[3], const float C[3], double g[3])
{
    const double ux = (double)B[0] - (double)A[0], uy = (double)B[1] - (double)A[1], uz = (double)B[2] - (double)A[2];
    const double wx = (double)C[0] - (double)A[0], wy = (double)C[1] - (double)A[1], wz = (double)C[2] - (double)A[2];
    const double yz = uy * wz, zy = uz * wy;
    const double zx = uz * wx, xz = ux * wz;
    const double xy = ux * wy, yx = uy * wx;
    g[0] = yz - zy;
    g[1] = zx - xz;
    g[2] = xy - yx;
}

// s += g: one corner's term of a vertex's sum
APD_HD void mesh_add(double s[3], const double g[3])
{
    s[0] = s[0] + g[0];
    s[1] = s[1] + g[1];
    s[2] = s[2] + g[2];
}

APD_HD void mesh_vertex_normal(const double s[3], float n[3])
{
    const double xx = s[0] * s[0], yy = s[1] * s[1], zz = s[2] * s[2];
    const double xy = xx + yy;
    const double len = sqrt(xy + zz);
    if (len > 0.0 && len <= 1.7976931348623157e308) {  // finite: a NaN fails the first test, +inf the second
        n[0] = (float)(s[0] / len);
        n[1] = (float)(s[1] / len);
        n[2] = (float)(s[2] / len);
    } else {
        n[0] = n[1] = n[2] = 0.0f;
    }
}

}  // namespace apd_fusion
