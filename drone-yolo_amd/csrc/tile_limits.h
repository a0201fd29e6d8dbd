// The limits of the cross-tile merge (tile_merge.hip) that the frame-mask assembly (mask_ops.hip) checks as well.
#pragma once

namespace dy {
constexpr int TM_MAX_SLOTS = 32768;  // K * max_det
constexpr int TM_MAX_KEEP = 4096;    // merge_max_det
}  // namespace dy
