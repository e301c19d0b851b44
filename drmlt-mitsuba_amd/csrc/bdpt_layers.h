// Layer indexing of the layered bidirectional film (drmlt_render_bdpt_layers, k_layers_bdpt), one copy for the host entry points
// and the kernel. A layer is a pair (depth d, s): d = s + t - 1 edges, 1 <= d <= maxDepth, 0 <= s <= d + 1 (t = d + 1 - s >= 0).
// Depth d has d + 2 layers, so the depths below it hold (d - 1)(d + 4) / 2 and D depths hold D (D + 5) / 2. Both answer -1
// outside these ranges and above BDPT_LAYERS_DEPTH_LIMIT, up to which the products stay within 32 bits.
#pragma once

#define BDPT_LAYERS_DEPTH_LIMIT 32767

__host__ __device__ inline int bdpt_layer_count(int max_depth) {
    return (max_depth < 1 || max_depth > BDPT_LAYERS_DEPTH_LIMIT) ? -1 : max_depth * (max_depth + 5) / 2;
}
__host__ __device__ inline int bdpt_layer_index(int depth, int s) {
    return (depth < 1 || depth > BDPT_LAYERS_DEPTH_LIMIT || s < 0 || s > depth + 1) ? -1 : (depth - 1) * (depth + 4) / 2 + s;
}
