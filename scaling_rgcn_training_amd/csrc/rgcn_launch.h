// rgcn_launch.h -- host-side launch helpers shared by the translation units of the library: the runtime -> compile-time
// ladders that pick a kernel instantiation.  Host code only: nothing here is, or changes, a __global__ / __device__ function.
//
//   for_padded_width   a padded width (16 / 32 / 64 / 128, see padded_width) as a compile-time constant; nest two for (KP, NP)
//   launch_row_groups  the row-per-lane-group kernels (segment sums, segment max): G lanes per row, 64 / G rows per wave,
//                      four waves per workgroup
#pragma once
#include <type_traits>
#include <utility>
#include "rgcn_common.h"

namespace rgcn {

// f(std::integral_constant<int, w>{}) for w = 16 / 32 / 64 / 128, whose int is returned; any other w is RGCN_ERR_WIDTH
template <class F>
inline int for_padded_width(int w, F&& f) {
    switch (w) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
    }
    return RGCN_ERR_WIDTH;
}

// lanes that share a row of width4 16-byte pieces (one piece per lane and step; rows wider than 32 pieces take several steps)
inline int lanes_per_row(int width4) { return width4 <= 4 ? 4 : (width4 <= 8 ? 8 : (width4 <= 16 ? 16 : 32)); }

// f(std::integral_constant<int, G>{}, grid) with G = lanes_per_row(width4) and the grid of 256-thread workgroups that gives
// every one of n_rows rows its lane group; returns f's int
template <class F>
inline int launch_row_groups(int width4, long n_rows, F&& f) {
    const int G = lanes_per_row(width4);
    const long waves = (n_rows + 64 / G - 1) / (64 / G);
    const dim3 grid((unsigned)((waves + 3) / 4));
    switch (G) {
        case 4: return f(std::integral_constant<int, 4>{}, grid);
        case 8: return f(std::integral_constant<int, 8>{}, grid);
        case 16: return f(std::integral_constant<int, 16>{}, grid);
        default: return f(std::integral_constant<int, 32>{}, grid);
    }
}

}  // namespace rgcn
