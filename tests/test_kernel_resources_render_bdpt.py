"""k_render_bdpt's registers, LDS and occupancy, read from the compiler's resource remarks of the build
(libdrmlt_amd.so.resources): it runs the bootstrap's evaluation with a film splat behind it and must not cost a wave for that."""
import os

from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_bdpt_fits_where_the_bootstrap_fits(native_lib):
    res = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(res), "the Makefile writes it next to the library"
    k = kernels(res)
    render = [r for n, r in k.items() if n.startswith("_Z13k_render_bdpt")]
    boot = [r for n, r in k.items() if n.startswith("_Z16k_bootstrap_bdpt")]
    assert len(render) == 1 and len(boot) == 1, sorted(k)
    render, boot = render[0], boot[0]
    print("k_render_bdpt: %d VGPRs + %d AGPRs, scratch %d B/lane, occupancy %d, static LDS %d B; k_bootstrap_bdpt: %d + %d, scratch %d B/lane, "
          "occupancy %d, static LDS %d B" % (render["VGPRs"], render["AGPRs"], render["ScratchSize"], render["Occupancy"], render["LDS"],
                                             boot["VGPRs"], boot["AGPRs"], boot["ScratchSize"], boot["Occupancy"], boot["LDS"]))
    assert render["VGPRs"] + render["AGPRs"] <= 256, render
    assert render["Occupancy"] >= boot["Occupancy"], (render, boot)
    assert render["LDS"] <= boot["LDS"], (render, boot)
