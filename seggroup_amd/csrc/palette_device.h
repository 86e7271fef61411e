// ScanNet's public class palette on the device (index 0 = unlabelled, white), r | g << 8 | b << 16: the 41 colours of
// seggroup_amd/visualize.py `colors`, shared by the coloured PLYs (kernels_visualize.hip) and the rendered images (kernels_render.hip).
#pragma once
#include <cstdint>

#include "seggroup_hip.h"

namespace sgpal {

static __constant__ uint32_t kPalette[SG_NUM_COLOURS + 1] = {
#define SG_RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
    SG_RGB(255, 255, 255), SG_RGB(174, 199, 232), SG_RGB(152, 223, 138), SG_RGB(31, 119, 180),  SG_RGB(255, 187, 120), SG_RGB(188, 189, 34),
    SG_RGB(140, 86, 75),   SG_RGB(255, 152, 150), SG_RGB(214, 39, 40),   SG_RGB(197, 176, 213), SG_RGB(148, 103, 189), SG_RGB(196, 156, 148),
    SG_RGB(23, 190, 207),  SG_RGB(178, 76, 76),   SG_RGB(247, 182, 210), SG_RGB(66, 188, 102),  SG_RGB(219, 219, 141), SG_RGB(140, 57, 197),
    SG_RGB(202, 185, 52),  SG_RGB(51, 176, 203),  SG_RGB(200, 54, 131),  SG_RGB(92, 193, 61),   SG_RGB(78, 71, 183),   SG_RGB(172, 114, 82),
    SG_RGB(255, 127, 14),  SG_RGB(91, 163, 138),  SG_RGB(153, 98, 156),  SG_RGB(140, 153, 101), SG_RGB(158, 218, 229), SG_RGB(100, 125, 154),
    SG_RGB(178, 127, 135), SG_RGB(120, 185, 128), SG_RGB(146, 111, 194), SG_RGB(44, 160, 44),   SG_RGB(112, 128, 144), SG_RGB(96, 207, 209),
    SG_RGB(227, 119, 194), SG_RGB(213, 92, 176),  SG_RGB(94, 106, 211),  SG_RGB(82, 84, 163),   SG_RGB(100, 85, 144)
#undef SG_RGB
};

}  // namespace sgpal
