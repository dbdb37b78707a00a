// onlineset.hpp — the grid constants of the online engine's two set kinds (online.hpp includes them; tests/onlineset_cases.py reads them here).
#pragma once
namespace pr {
constexpr int ONLINESET_NB_FUSED = 512;      // most workgroups of the fused rows kernel: NB = min(capacity, ONLINESET_NB_FUSED), one entry per stride
constexpr int ONLINESET_NB_DELIGHT = 64;     // most workgroups of the DELIGHT rows kernel: NB = min(ceil(capacity / 16), ONLINESET_NB_DELIGHT), 16 entries per stride
}  // namespace pr
