// apd_mesh_host.h -- the mesh object (apd_mesh_t of include/apd_mi355x.h), seen by who makes one (apd_volume.hip: extraction) and by
// who owns its life, its files and its cleaning (apd_mesh.hip) and its simplification (apd_mesh_simplify.hip).
#pragma once

#include <stdint.h>

// An indexed triangle mesh in device memory on `device`; every array is the object's own (hipMalloc) or null where its count is 0
struct apd_mesh {
    int device = 0;
    long long vertices = 0, faces = 0;
    int colour = 0, normals = 0;
    float *xyz = nullptr;      // 3 per vertex
    uint8_t *bgr = nullptr;    // 3 per vertex, with colour
    float *normal = nullptr;   // 3 per vertex, with normals
    int32_t *index = nullptr;  // 3 per face, each in [0, vertices)
};
