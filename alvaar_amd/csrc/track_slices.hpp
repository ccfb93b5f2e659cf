// How the compaction of the slot-wise tracking step (track_compact_device.hpp) cuts a frame's n slots among its workgroups.  Plain C++
// (constexpr: usable in device code as well), so that a host-only test can check the rule for every n (tests/cpp/track_slices.cpp).
#pragma once

constexpr int CMP_NT = 256, CMP_MAX_WG = 32;

// Workgroup g of G owns the slots [g * per, min(n, (g + 1) * per)), per a multiple of the wave size.  The slices cover [0, n); the
// last ones may be empty unless the grid comes from track_pose_all_grid.
constexpr int track_slice_len(int n, int G) { return ((n + G - 1) / G + 63) / 64 * 64; }

// k_track_compact: ~CMP_NT slots per workgroup, at most CMP_MAX_WG workgroups (a workgroup with an empty slice only arrives)
constexpr int track_compact_grid(int n) {
    const int g = (n + CMP_NT - 1) / CMP_NT;
    return g < 1 ? 1 : g > CMP_MAX_WG ? CMP_MAX_WG : g;
}

// The compaction phase of the fused pose launch (pnp.hip k_pose_all): at most 96 workgroups of 64-slot slices, longer slices past 6144
// slots.  Every slice is non-empty -- a workgroup arrives on the gather counter from inside its slice, so the gathered-seq word waits
// for all G -- and holds at most 512 slots (one slot per thread) for n <= 49152.
constexpr int track_pose_all_grid(int n) {
    const int per = ((n + 95) / 96 + 63) / 64 * 64;
    return per > 0 ? (n + per - 1) / per : 1;
}
