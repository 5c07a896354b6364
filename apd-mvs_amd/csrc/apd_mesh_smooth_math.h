// apd_mesh_smooth_math.h -- what the vertex adjacency of an indexed triangle mesh is and what smoothing over it computes (arithmetic
// contract C24): the rules under apd_mesh_adjacency and apd_mesh_smooth, written once and compiled by hipcc into the
// kernels (apd_mesh_smooth.hip) and by the host compiler into the sequential checker (tests/helpers/mesh_smooth_ref.cpp).  As in
// apd_mesh_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order.
//
// Adjacency (integers only).  Every face (a, b, c) gives the six directed pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c)
// (smooth_face_keys); a pair with equal ends is dropped -- a face may repeat an index.  The neighbours of v are the distinct w of its
// pairs in ascending order; the multiplicity of the edge {v, w} is the number of times the pair (v, w) occurs, which is the number of
// face sides on the edge.  Multiplicity 1: a boundary edge; 3 or more: a non-manifold edge; a vertex is a boundary vertex when one
// of its edges is a boundary edge.  A vertex no face names has no neighbours and is not a boundary vertex.  Two equal faces give
// their edges multiplicity 2: a duplicate closes what a single face leaves open.
//
// One step with a factor k (a float, widened to binary64) from positions p to positions p'.  Neighbour w of v contributes when the
// three coordinates of p[w] are finite (smooth_finite) and the boundary mode takes it (smooth_takes): under ALONG a boundary vertex
// takes only the neighbours across its boundary edges, under FIXED a boundary vertex does not move (smooth_held), under FREE a boundary
// vertex is treated as any other.  A vertex moves when it is not held, its own position is finite and at least one neighbour
// contributes.  For a vertex that moves, per coordinate: s = the binary64 sum of (double)p[w] over the contributing neighbours in
// ascending w, from +0.0 (smooth_add); m = s / (double)count; p'[v] = (float)((double)p[v] + k * (m - (double)p[v])) (smooth_place).
// For every other vertex p'[v] = p[v], the same bits.
//
// An iteration is a step with lambda, followed, when mu != 0, by a step with mu: mu = 0 is plain Laplacian smoothing, lambda = 0.5
// with mu = -0.53 is Taubin's pair.  Every step reads only the positions of the step before it; the adjacency and the boundary
// flags come from the connectivity and are the same in every step.  `moved` is the number of vertices that move in the first step.
#pragma once

#include <math.h>
#include <stdint.h>

#include "apd_fusion_math.h"

namespace apd_fusion {

constexpr int kSmoothFixed = 0, kSmoothAlong = 1, kSmoothFree = 2;  // APD_SMOOTH_BOUNDARY_FIXED, _ALONG, _FREE
constexpr uint64_t kSmoothNoPair = ~(uint64_t)0;                    // the key of a dropped pair: above every pair, vertices are fewer than 2^31
constexpr uint32_t kSmoothBoundaryEdge = 0x80000000u;               // in an entry of a neighbour list: the edge to that neighbour has multiplicity 1

// The key of the directed pair (v, w): ascending keys are ascending v and within v ascending w
APD_HD uint64_t smooth_pair_key(int32_t v, int32_t w) { return v == w ? kSmoothNoPair : ((uint64_t)(uint32_t)v << 32) | (uint64_t)(uint32_t)w; }

APD_HD void smooth_face_keys(int32_t a, int32_t b, int32_t c, uint64_t key[6])
{
    key[0] = smooth_pair_key(a, b);
    key[1] = smooth_pair_key(b, a);
    key[2] = smooth_pair_key(b, c);
    key[3] = smooth_pair_key(c, b);
    key[4] = smooth_pair_key(c, a);
    key[5] = smooth_pair_key(a, c);
}

// The entry of neighbour w in a vertex's list, for an edge of this multiplicity (>= 1)
APD_HD uint32_t smooth_entry(uint32_t w, uint32_t multiplicity) { return multiplicity == 1u ? (w | kSmoothBoundaryEdge) : w; }
APD_HD uint32_t smooth_entry_vertex(uint32_t entry) { return entry & ~kSmoothBoundaryEdge; }
APD_HD bool smooth_entry_boundary(uint32_t entry) { return (entry & kSmoothBoundaryEdge) != 0u; }
APD_HD bool smooth_nonmanifold(uint32_t multiplicity) { return multiplicity >= 3u; }

APD_HD bool smooth_finite(float x, float y, float z)
{
    const float top = 3.4028234663852886e38f;  // a NaN fails each test
    return fabsf(x) <= top && fabsf(y) <= top && fabsf(z) <= top;
}

// A vertex the mode holds in place
APD_HD bool smooth_held(int mode, bool boundary_vertex) { return mode == kSmoothFixed && boundary_vertex; }

// Whether the mode lets a vertex take the neighbour of this entry
APD_HD bool smooth_takes(int mode, bool boundary_vertex, uint32_t entry) { return !(mode == kSmoothAlong && boundary_vertex) || smooth_entry_boundary(entry); }

APD_HD void smooth_add(double s[3], float x, float y, float z)
{
    s[0] = s[0] + (double)x;
    s[1] = s[1] + (double)y;
    s[2] = s[2] + (double)z;
}

// One coordinate of a vertex that moves: p its own, s the sum over `count` >= 1 contributing neighbours
APD_HD float smooth_place(float p, double s, uint32_t count, double k)
{
    const double m = s / (double)count;
    const double d = m - (double)p;
    const double step = k * d;
    return (float)((double)p + step);
}

}  // namespace apd_fusion
