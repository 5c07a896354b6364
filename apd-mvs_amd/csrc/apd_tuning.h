// apd_tuning.h -- the build-time parameters of the kernels that a recorded run has varied.
//
// The rule: a parameter is a macro here only if a committed file under profiles/ records a run that varied it, or a script
// under tools/ varies it; its comment names that file.  The macro exists so that tools/tune.sh can rebuild the library with
// another value (-DAPD_X=...) and repeat that run -- nothing in the product sets one, and the library reads nothing from the
// environment.  Every other constant is a named constexpr beside its use, and an on/off experiment that has been decided
// leaves the sources with its losing arm (DESIGN.md section 4 lists what went where).  Parameters that name a constant of a
// kernel file (kWaveH, kFwLds) are expanded where that file uses them.
#pragma once

// ---- apd_device.h ----
#ifndef APD_ROW_PREFETCH
#define APD_ROW_PREFETCH 1  // rows of gathers in flight ahead of the row being reduced (profiles/r02/tune_scratch.txt)
#endif

// ---- apd_sweep.h ----
#ifndef APD_CB_ROWS
#define APD_CB_ROWS 4  // pixel rows of a wave's checkerboard footprint (profiles/r01/tuning/tune_rows.txt)
#endif
#ifndef APD_FF_ROWS
#define APD_FF_ROWS 8  // pixel rows of a wave's block in the full-frame kernels (profiles/r01/tuning/tune_rows.txt); the windowed K14/K15 need 8
#endif

// ---- apd_kernels_k67w.hip ----
#ifndef APD_WIN_H
#define APD_WIN_H (kWaveH + 16)   // rows of fetch positions: footprint + 2 * (patch radius 5 + 3 texels of slack) (profiles/r02/tune_win_h.txt)
#endif
#ifndef APD_K67W_WAVES
#define APD_K67W_WAVES 4  // waves per SIMD (profiles/r02/tune_scratch.txt, profiles/r02/tune_k67_waves5.txt)
#endif
#ifndef APD_K67W_WAVES_F32
#define APD_K67W_WAVES_F32 3  // float windows: three waves per SIMD also with the single-texel entries (4 waves, 128 VGPRs: 32.4 against 29.1 ms
                              // for the first iteration at 2048x1536, 16.0 against 14.6 later; profiles/r03/tune_float_windows.txt)
#endif

// ---- apd_kernels_k1415w.hip ----
#ifndef APD_FW_TILE_PITCH
#define APD_FW_TILE_PITCH (kFwLds + 1)  // floats per row of the reference tile (profiles/r01/tuning/tune_k1415_win_pitch.txt)
#endif
#ifndef APD_K1415_WIN_PITCH
#define APD_K1415_WIN_PITCH 72  // entries per window row: a 32-lane group reads four rows of eight columns (apd_window.h; profiles/r01/tuning/tune_k1415_win_pitch.txt)
#endif
#ifndef APD_K14_WIN_H
#define APD_K14_WIN_H 32  // rows of fetch positions: 8 + 2 * (patch radius 5 + 7 texels of slack) (profiles/r01/tuning/tune_k1415_win_pitch.txt)
#endif
// K14 walks the (sample, lane) pairs of a chunk 64 at a time instead of one sample per wave-level NCC ...
#ifndef APD_K14_PAIRS_FROM_N
#define APD_K14_PAIRS_FROM_N 10  // ... in launches with at least this many source views (float images; profiles/r05/tune_k14.txt)
#endif
#ifndef APD_K14_PAIRS_FROM_N_PHOTO
#define APD_K14_PAIRS_FROM_N_PHOTO 8   // ... 8-bit input, photometric passes (profiles/r06/ab_k14_pairs_by_pass_kind.txt)
#endif
#ifndef APD_K14_PAIRS_FROM_N_GEOM
#define APD_K14_PAIRS_FROM_N_GEOM 2    // ... 8-bit input, passes with the geometric term (same file)
#endif
#ifndef APD_K14_PAIRS_MIN_SAVE
#define APD_K14_PAIRS_MIN_SAVE 2  // photometric passes: a chunk walks its (sample, lane) pairs when that saves at least this many wave-level NCCs (geometric: one;
                                  // profiles/r06/ab_k14_pairs_by_pass_kind.txt)
#endif
#ifndef APD_K14_CHUNK
#define APD_K14_CHUNK 8  // depth samples per staged window = length of the register vector of cost sums: 4, 8 or 16 (K14 ms at 6200x4130, 10 views,
                         // photometric / geometric pass, profiles/r05/tune_k14.txt: 4: 316 / 276, 8: 286 / 275, 16: 377 / 448)
#endif
#ifndef APD_K14W_WAVES
#define APD_K14W_WAVES 4  // ms at 4096x3072, 8 views: 4 waves/SIMD (128 VGPRs, 18 spilled) 140.6, 3 waves 150.1
                          // the (sample, lane)-pair variant, 6200x4130, 10 views: 4 waves (42 spilled) 295.2 / 361.3 ms (photometric / geometric pass), 3 waves (164 VGPRs, none) 306.9 / 388.7 (profiles/r04/ab_k14_pairs_waves.txt)
#endif
#ifndef APD_K1415W_WAVES_F32
#define APD_K1415W_WAVES_F32 3  // float windows (single-texel entries, 9.5 KB per wave like the 8-bit ones); ms at 2048x1536, 8 views, K14 / K15:
                                // 2 waves/SIMD 41.6 / 3.77, 3 waves 34.5 / 3.18, 4 waves 36.5 / 3.87 (8-byte pair entries, 2 waves: 40.4 / 3.80;
                                // profiles/r03/tune_float_windows.txt)
#endif

// ---- apd_kernels_weak.hip ----
#ifndef APD_WEAK_SUPER_SHIFT
#define APD_WEAK_SUPER_SHIFT 4  // log2 of the supertile edge, in tiles, of the WEAK list order (profiles/r03/ab_k910_list_order.txt)
#endif
#ifndef APD_K910_WIN_H
#define APD_K910_WIN_H 28  // rows of fetch positions of the centre-patch window (profiles/r03/ab_k910_centre_window.txt)
#endif
#ifndef APD_K910_WAVES
#define APD_K910_WAVES 2  // waves per SIMD (profiles/r02/tune_k910_waves.txt, profiles/r03/ab_k910_list_order.txt)
#endif

// ---- apd_mesh_render.hip ----
#ifndef APD_MESH_RENDER_SPLIT
#define APD_MESH_RENDER_SPLIT 64  // pixels of a face's clipped bounding box above which waves draw it instead of a lane; work ms of a render into
                                  // 3200 x 2400 at 64 / 256 / 1024: a million 5-pixel faces 2.10 / 2.09 / 2.08, 78 thousand 58-pixel faces 2.20 / 2.24 /
                                  // 2.83, 12 thousand 359-pixel faces 2.13 / 2.38 / 3.47 (tools/mesh_render_time.py with apd_mesh_render_split,
                                  // profiles/mesh_render/timing.txt)
#endif
