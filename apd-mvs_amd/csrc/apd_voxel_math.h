// apd_voxel_math.h -- the cell and the key of a point in the cubic grid of apd_points_merge_voxels (arithmetic contract C10,
// DESIGN.md), written once and compiled by hipcc into the merge (apd_points_merge.hip) and by the host compiler into whoever
// restates it.  As in apd_fusion_math.h: -ffp-contract=off, no fast-math, every operation an IEEE operation in a fixed order.
#pragma once

#include "apd_fusion_math.h"

namespace apd_fusion {

constexpr int kVoxelAxisBits = 21;                        // bits of one axis in the key
constexpr int kVoxelHalf = 1 << (kVoxelAxisBits - 1);     // cells of an axis are -2^20 .. 2^20 - 1

// The cell of coordinate x on one axis: floorf((x - origin) / size), a binary32 subtraction and an IEEE division.  False -- the
// point is dropped -- when the floor is not in [-2^20, 2^20): too far out, infinite, or NaN (which fails both comparisons).
APD_HD bool voxel_cell(float x, float origin, float size, int &cell)
{
    const float t = (x - origin) / size;
    const float f = floorf(t);
    if (!(f >= -(float)kVoxelHalf && f < (float)kVoxelHalf)) {
        return false;
    }
    cell = (int)f;
    return true;
}

// The key of point P: z, y, x cells, biased by 2^20, in bits 42-62, 21-41, 0-20.  Ascending keys are z-major.  False: dropped.
APD_HD bool voxel_key(const float P[3], const float origin[3], float size, uint64_t &key)
{
    int c[3];
    for (int a = 0; a < 3; ++a) {
        if (!voxel_cell(P[a], origin[a], size, c[a])) {
            return false;
        }
    }
    key = ((uint64_t)(c[2] + kVoxelHalf) << (2 * kVoxelAxisBits)) | ((uint64_t)(c[1] + kVoxelHalf) << kVoxelAxisBits) |
          (uint64_t)(c[0] + kVoxelHalf);
    return true;
}

}  // namespace apd_fusion
