// The UMI correction on BUS records (pa_bus_umi_correct) as csrc/bus_umi.hip builds it: the thresholds of its neighbour search. Neither value was
// varied yet; what is measured is the block bin's LDS search against the HBM variant on the same barcodes.
#pragma once
#include <cstdint>

namespace pa {

constexpr uint32_t UM_BLOCK = 256;          // threads of a block (4 waves)
constexpr uint32_t UM_LANE_MAX = 64;        // a barcode of up to this many molecules: a lane per molecule compares its UMI with every other one of the barcode
constexpr uint32_t UM_LDS_CAP = 8192;       // a barcode of up to this many molecules: one block, its UMIs in LDS (64 KiB of u64 words: two blocks share a CU's 160 KiB; 32 KiB of u32 words); above: searched in HBM

}  // namespace pa
