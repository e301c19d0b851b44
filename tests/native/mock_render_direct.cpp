// drmlt_node_render_direct for the recording stand-ins of libdrmlt_amd.so that were written before the adaptor could call it
// (adaptor_harness.cpp -DMOCK_ABI, conductor_harness.cpp): linked beside them so that the adaptor resolves. None of them sets directPass=device; a call is answered as a failure, never as an image.
#include "drmlt_abi.h"

extern "C" int drmlt_node_render_direct(drmlt_node *, int32_t, int32_t, uint64_t, float *) { return DRMLT_E_INVALID; }
