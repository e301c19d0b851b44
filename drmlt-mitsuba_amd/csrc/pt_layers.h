// Layer indexing of the layered path-traced film (drmlt_render_pt_layers, k_render_pt_layers), one copy for the host entry points
// and the kernel. A layer is a pair (depth d, strategy): d edges from the camera to the emitter, 1 <= d <= maxDepth; strategy
// DRMLT_PT_HIT = 0 (the BSDF-sampled ray found the emitter) or DRMLT_PT_DIRECT = 1 (the light sample). Both answer -1 outside
// these ranges and above PT_LAYERS_DEPTH_LIMIT, up to which the products stay within 32 bits.
#pragma once

#define PT_LAYERS_DEPTH_LIMIT 0x3fffffff
// k_render_pt_layers holds a sample's terms in LDS until the sample ends: (6 maxDepth + 1) floats per lane, 37 KB per wave at
// bdpt's bound (BDPT_MAX_DEPTH, device_types.h), which is the bound here too
#define PT_LAYERS_MAX_DEPTH 24

__host__ __device__ inline int pt_layer_count(int max_depth) {
    return (max_depth < 1 || max_depth > PT_LAYERS_DEPTH_LIMIT) ? -1 : 2 * max_depth;
}
__host__ __device__ inline int pt_layer_index(int depth, int strategy) {
    return (depth < 1 || depth > PT_LAYERS_DEPTH_LIMIT || strategy < 0 || strategy > 1) ? -1 : 2 * (depth - 1) + strategy;
}
