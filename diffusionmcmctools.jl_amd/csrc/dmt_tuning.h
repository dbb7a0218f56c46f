// dmt_tuning.h — the kernels' build-time numeric tunables, each with the measurement that chose
// its default (profiles/…, DESIGN.md §6–§9).  Override one with
//   make variants VARIANT_FLAGS=-DDMT_KCHUNK=8 VARIANT_NAME=k8
// Every value gives the same results; the static_asserts state the legal ones.  One more lives
// in dmt_internal.h because the runtime lays the paths out by it: DMT_PATH_PACKET (fp32
// lane-packet length in points: 32, or 16 = one staged piece).
// The other build-time switches are measurement builds with unchanged results: DMT_PC_STAMPS
// (scripts/pc_stamps.py), DMT_SVC_PROBE (scripts/svc_probe.py), DMT_AUX_CHECK
// (scripts/td_fault_probe.py).
#pragma once
#include "dmt_internal.h"

// lane kernels: steps per prefetch chunk.  One chunk of 8 measured the same as two of 4 on C3
// (1 007–1 008 vs 1 001–1 013 µs per draw, profiles/r05h)
#ifndef DMT_KCHUNK
#define DMT_KCHUNK 4
#endif
static_assert(DMT_KCHUNK >= 4 && 64 % DMT_KCHUNK == 0 && 2 * DMT_KCHUNK <= dmt::kPadPoints,
              "DMT_KCHUNK: 4, 8 or 16 (the prefetch reads up to 2 chunks past a segment end)");

// packet kernels: their guiding-term chunk.  8 measured the same on C5 (1 431–1 438 vs
// 1 434–1 440 µs, profiles/r05i): C5 does not wait on its H, F loads
#ifndef DMT_PK_KCHUNK
#define DMT_PK_KCHUNK DMT_KCHUNK
#endif
static_assert(DMT_PK_KCHUNK >= 4 && dmt::kPkChunkPts % DMT_PK_KCHUNK == 0,
              "DMT_PK_KCHUNK: 4, 8 or 16 (whole chunks per staged piece, whole 16-byte pieces per chunk)");

// pair kernels' chunk, doubled when it would hold an odd number of Philox blocks (Lorenz fp32,
// 3 normals per step → 8 steps); the pair mapping measured no faster
#ifndef DMT_KCHUNK_PAIR_BASE
#define DMT_KCHUNK_PAIR_BASE 4
#endif
static_assert(DMT_KCHUNK_PAIR_BASE == 4 || DMT_KCHUNK_PAIR_BASE == 8,
              "DMT_KCHUNK_PAIR_BASE: 4 or 8 (twice its double stays within the tile's spare rows)");

// k_block_ps: steps per producer → consumer hand-off (8 with two workgroups per CU, no spills,
// measured no better: 1 877 vs 1 749–1 782 µs on C5)
#ifndef DMT_PS_CHUNK
#define DMT_PS_CHUNK 16
#endif
static_assert(DMT_PS_CHUNK >= 4 && DMT_PS_CHUNK <= 32 && DMT_PS_CHUNK % 4 == 0,
              "DMT_PS_CHUNK: a multiple of the consumer's 4-step chunk, at most 32 (the hand-off's LDS)");

// k_block_ps_pk: the consumer's H, F register ring in chunks (2 = one ahead; 4, three ahead,
// measured the same: 1 350 vs 1 341–1 343 µs, profiles/r05l)
#ifndef DMT_PSPK_RING
#define DMT_PSPK_RING 2
#endif
static_assert(DMT_PSPK_RING == 2 || DMT_PSPK_RING == 4,
              "DMT_PSPK_RING: 2 or 4 (a ring of whole packets)");

// k_block_wave: wave S reads its LDS rows this many steps ahead in the straight-line chunk
// (4 and 8 measured slower: 1 343–1 370 and 1 375–1 396 µs per 10⁴ steps, profiles/r05g)
#ifndef DMT_S_AHEAD
#define DMT_S_AHEAD 2
#endif
static_assert(DMT_S_AHEAD >= 1 && DMT_S_AHEAD <= 8, "DMT_S_AHEAD: 1 to 8 steps");

// k_mcmc_resident_pc: Philox blocks + Box–Muller the producer interleaves at a time
#ifndef DMT_PC_DRAW_GROUP
#define DMT_PC_DRAW_GROUP 8
#endif
static_assert(DMT_PC_DRAW_GROUP >= 1, "DMT_PC_DRAW_GROUP: a positive number of Philox blocks");

// k_mcmc_resident_pc with one producer: steps of every 8-step lane run whose normals the
// consumer draws itself (1: the same as 2, 3: 7.3e10, 4: 6.0e10 against 7.95–8.17e10 path
// steps/s at 200 iterations, profiles/r02zc, r02ze)
#ifndef DMT_PC_CONS_STEPS
#define DMT_PC_CONS_STEPS 2
#endif
static_assert(DMT_PC_CONS_STEPS >= 0 && DMT_PC_CONS_STEPS <= 4,
              "DMT_PC_CONS_STEPS: 0 to 4 of a lane run's 8 steps");

// row-layout lane kernels: chunks loaded ahead (0: two when a chunk's inputs fit in 40
// registers per lane, e.g. FHN, else one).  C3: two chunks 1 001–1 013 vs one 1 061–1 084 µs per
// draw; three slower, 1 036–1 042 (profiles/r05h, r05i, r05r)
#ifndef DMT_LANE_AHEAD
#define DMT_LANE_AHEAD 0
#endif
static_assert(DMT_LANE_AHEAD >= 0 && DMT_LANE_AHEAD <= 2, "DMT_LANE_AHEAD: 0 (auto), 1 or 2");

// lane kernels' X°/W° stores: 0 plain, 1 nontemporal, 2 nontemporal for fp64 only.  Nontemporal
// stores take C3 (fp64) from 1 239 to 1 144 µs per draw but C5 (fp32, whose mixed-selector
// stores write partial lines) from 1 878 to 1 957 µs (profiles/r03f)
#ifndef DMT_LANE_NT_STORES
#define DMT_LANE_NT_STORES 2
#endif
static_assert(DMT_LANE_NT_STORES >= 0 && DMT_LANE_NT_STORES <= 2, "DMT_LANE_NT_STORES: 0, 1 or 2");
