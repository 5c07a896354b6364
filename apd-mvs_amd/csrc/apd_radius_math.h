// apd_radius_math.h -- who is whose neighbour within a radius (arithmetic contract C11): the relation under
// apd_points_neighbour_counts and apd_points_remove_sparse, written once and compiled by hipcc into the count kernel
// (apd_points_radius.hip) and by the host compiler into whoever restates it.  As in apd_voxel_math.h: -ffp-contract=off, no
// fast-math, every operation an IEEE binary32 operation in a fixed order.
//
// Grid.  Cubic, cell size `radius`, origin `origin` (0, 0, 0 when the caller gives none).  The cell of a point on each axis is
// voxel_cell(x, origin, radius) of contract C10.  A point for which voxel_key is false -- a non-finite coordinate, a cell beyond
// +-2^20 -- is OUTSIDE THE GRID: it has no neighbours and is nobody's neighbour.
//
// Neighbour.  Point j is a neighbour of point i when
//   j != i as indices (two points at one position are each other's neighbours),
//   both are inside the grid,
//   their cells differ by at most 1 on every axis,
//   d2(i, j) <= r2, with d2 = (dx * dx + dy * dy) + dz * dz, dx = x_i - x_j and so on, and r2 = radius * radius.
// The relation is symmetric: x_j - x_i is the exact negation of x_i - x_j and the squares do not see the sign.
//
// The cell condition makes the search of the 27 cells around a point THE DEFINITION and not an approximation of a ball: a loop
// over all pairs that applies radius_neighbour gives the same integers as the grid search, whatever the rounding below does.
// What the condition costs: in real arithmetic nothing -- d2 <= r2 gives |dx| <= radius, so the two quotients (x - origin) /
// radius differ by at most 1 and their floors by at most 1.  In binary32 the quotient carries the rounding of the subtraction and
// of the division: half a unit in the last place each, which is 2^-24 of a cell near cell 1 and grows to about 1/8 of a cell at
// cell 2^20.  Rounding is monotonic, so a pair whose dx is well inside the radius keeps floors one apart; only a pair within that
// rounding of EXACTLY one radius apart along an axis can land two cells apart, and such a pair is then not counted -- by every
// implementation alike, since all of them test the cells.  With origin 0 and a radius that is a power of two the quotient is
// exact and the condition never binds.
//
// Count.  count_i = min(number of neighbours of i, cap); cap == 0: no cap.  It does not depend on the order in which candidates
// are visited, so a search may stop at `cap`.
// Removal.  Point i is kept when its uncapped count is >= min_neighbours -- the same as its count with cap = min_neighbours
// reaching min_neighbours.  min_neighbours == 0 keeps every point, those outside the grid too.
//
// Cost.  The work is the number of (point, candidate in the 27 cells around it) pairs: with cap == 0 a cell of m members costs
// m * m distance tests; with a cap a point in a dense region stops after `cap` hits.
#pragma once

#include "apd_voxel_math.h"

namespace apd_fusion {

// The three cells of point P; false: outside the grid
APD_HD bool radius_cells(const float P[3], const float origin[3], float radius, int cell[3])
{
    for (int a = 0; a < 3; ++a) {
        if (!voxel_cell(P[a], origin[a], radius, cell[a])) {
            return false;
        }
    }
    return true;
}

// voxel_key's packing of three cells in [-2^20, 2^20), and back
APD_HD uint64_t radius_key(int cx, int cy, int cz)
{
    return ((uint64_t)(cz + kVoxelHalf) << (2 * kVoxelAxisBits)) | ((uint64_t)(cy + kVoxelHalf) << kVoxelAxisBits) | (uint64_t)(cx + kVoxelHalf);
}

APD_HD void radius_cells_of_key(uint64_t key, int cell[3])
{
    const uint64_t mask = ((uint64_t)1 << kVoxelAxisBits) - 1;
    cell[0] = (int)(key & mask) - kVoxelHalf;
    cell[1] = (int)((key >> kVoxelAxisBits) & mask) - kVoxelHalf;
    cell[2] = (int)((key >> (2 * kVoxelAxisBits)) & mask) - kVoxelHalf;
}

APD_HD bool radius_cells_adjacent(const int a[3], const int b[3])
{
    for (int c = 0; c < 3; ++c) {
        const int d = a[c] - b[c];
        if (d < -1 || d > 1) {
            return false;
        }
    }
    return true;
}

APD_HD float radius_d2(const float A[3], const float B[3])
{
    const float dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// d2 <= r2: false for a NaN d2 (inf - inf of two far points inside the grid cannot happen: they are finite)
APD_HD bool radius_within(const float A[3], const float B[3], float r2) { return radius_d2(A, B) <= r2; }

// The relation for two distinct points inside the grid with cells ca and cb
APD_HD bool radius_neighbour(const float A[3], const int ca[3], const float B[3], const int cb[3], float r2)
{
    return radius_cells_adjacent(ca, cb) && radius_within(A, B, r2);
}

}  // namespace apd_fusion
