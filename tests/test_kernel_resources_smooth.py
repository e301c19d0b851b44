"""The chain kernels' registers with vertex normals in the path step, against the numbers of the commit before it (its
libdrmlt_amd.so.resources, pinned in BUILDS below: the parent's occupancy in waves per SIMD, its VGPRs + AGPRs and scratch bytes per
lane, and the VGPRs + AGPRs measured for this commit).
  - A build without feature bit 4 compiles none of the new code: its three numbers are the parent's exactly.
  - A build with bit 4 keeps at least the parent's occupancy and takes no more registers than measured here. That is a departure from
    "no more than the parent": the smooth branch is not register-neutral. Where a build is not capped it takes 1 to 4 registers more
    than the parent's (k_mutate_v3<15>: 8 and 9, at two waves either way); no build loses a wave, the builds capped at 168 stay there,
    and k_mutate_v5<7> with its rows in memory still spills nothing. The scratch size is printed beside the parent's (reported, not
    bounded here; tests/test_kernel_resources.py bounds the builds it names): the k_mutate_v5<15> builds with rows in memory spill
    204 / 164 / 164 B where the parent spilled 164 / 168 / 168 B."""
import os
import re

from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (parent occupancy, parent VGPRs + AGPRs, parent scratch, VGPRs + AGPRs of this commit)
BUILDS = {
    "_Z11k_mutate_v3ILi0ELb1EEv7DParamsjj": (2, 197, 0, 197),
    "_Z11k_mutate_v3ILi15ELb0EEv7DParamsjj": (2, 224, 0, 232),
    "_Z11k_mutate_v3ILi15ELb1EEv7DParamsjj": (2, 226, 0, 235),
    "_Z11k_mutate_v3ILi3ELb1EEv7DParamsjj": (2, 216, 0, 216),
    "_Z11k_mutate_v3ILi7ELb1EEv7DParamsjj": (2, 218, 0, 221),
    "_Z11k_mutate_v4ILi0ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 157, 0, 157),
    "_Z11k_mutate_v4ILi0ELb1ELb1ELb0ELb0EEv7DParamsjj": (2, 173, 0, 173),
    "_Z11k_mutate_v4ILi15ELb0ELb0ELb0ELb1EEv7DParamsjj": (2, 195, 0, 199),
    "_Z11k_mutate_v4ILi15ELb0ELb0ELb1ELb0EEv7DParamsjj": (2, 191, 0, 194),
    "_Z11k_mutate_v4ILi15ELb0ELb0ELb1ELb1EEv7DParamsjj": (2, 195, 0, 198),
    "_Z11k_mutate_v4ILi15ELb0ELb1ELb1ELb0EEv7DParamsjj": (2, 191, 0, 195),
    "_Z11k_mutate_v4ILi15ELb1ELb0ELb0ELb1EEv7DParamsjj": (2, 202, 0, 205),
    "_Z11k_mutate_v4ILi15ELb1ELb0ELb1ELb0EEv7DParamsjj": (2, 198, 0, 201),
    "_Z11k_mutate_v4ILi15ELb1ELb0ELb1ELb1EEv7DParamsjj": (2, 202, 0, 205),
    "_Z11k_mutate_v4ILi16ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 165, 0, 165),
    "_Z11k_mutate_v4ILi16ELb1ELb1ELb0ELb0EEv7DParamsjj": (2, 169, 0, 169),
    "_Z11k_mutate_v4ILi19ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 159, 0, 159),
    "_Z11k_mutate_v4ILi23ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 164, 0, 167),
    "_Z11k_mutate_v4ILi32ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 139, 0, 139),
    "_Z11k_mutate_v4ILi32ELb1ELb1ELb0ELb0EEv7DParamsjj": (3, 143, 0, 143),
    "_Z11k_mutate_v4ILi3ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 163, 0, 163),
    "_Z11k_mutate_v4ILi3ELb1ELb1ELb0ELb0EEv7DParamsjj": (2, 188, 0, 188),
    "_Z11k_mutate_v4ILi48ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 134, 0, 134),
    "_Z11k_mutate_v4ILi48ELb1ELb1ELb0ELb0EEv7DParamsjj": (3, 138, 0, 138),
    "_Z11k_mutate_v4ILi7ELb0ELb0ELb0ELb0EEv7DParamsjj": (3, 167, 0, 168),
    "_Z11k_mutate_v4ILi7ELb1ELb0ELb0ELb0EEv7DParamsjj": (3, 167, 0, 168),
    "_Z11k_mutate_v4ILi8ELb0ELb0ELb0ELb1EEv7DParamsjj": (2, 174, 0, 174),
    "_Z11k_mutate_v4ILi8ELb0ELb0ELb1ELb0EEv7DParamsjj": (2, 169, 0, 169),
    "_Z11k_mutate_v5ILi0ELb1ELb0ELb0ELb1ELb0EEv7DParamsjj": (3, 165, 0, 165),
    "_Z11k_mutate_v5ILi0ELb1ELb0ELb0ELb1ELb1EEv7DParamsjj": (3, 167, 0, 167),
    "_Z11k_mutate_v5ILi0ELb1ELb0ELb1ELb1ELb0EEv7DParamsjj": (2, 187, 0, 187),
    "_Z11k_mutate_v5ILi15ELb0ELb1ELb0ELb0ELb0EEv7DParamsjj": (2, 222, 0, 224),
    "_Z11k_mutate_v5ILi15ELb0ELb1ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 164, 168),
    "_Z11k_mutate_v5ILi15ELb1ELb0ELb0ELb0ELb0EEv7DParamsjj": (2, 219, 0, 221),
    "_Z11k_mutate_v5ILi15ELb1ELb0ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 168, 168),
    "_Z11k_mutate_v5ILi15ELb1ELb1ELb0ELb0ELb0EEv7DParamsjj": (2, 224, 0, 226),
    "_Z11k_mutate_v5ILi15ELb1ELb1ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 168, 168),
    "_Z11k_mutate_v5ILi1ELb1ELb0ELb0ELb1ELb0EEv7DParamsjj": (2, 171, 0, 171),
    "_Z11k_mutate_v5ILi1ELb1ELb0ELb0ELb1ELb1EEv7DParamsjj": (3, 168, 0, 168),
    "_Z11k_mutate_v5ILi3ELb1ELb0ELb0ELb1ELb0EEv7DParamsjj": (2, 173, 0, 173),
    "_Z11k_mutate_v5ILi3ELb1ELb0ELb0ELb1ELb1EEv7DParamsjj": (3, 168, 0, 168),
    "_Z11k_mutate_v5ILi7ELb1ELb0ELb0ELb0ELb0EEv7DParamsjj": (2, 178, 0, 181),
    "_Z11k_mutate_v5ILi7ELb1ELb0ELb0ELb1ELb0EEv7DParamsjj": (2, 179, 0, 182),
    "_Z11k_mutate_v5ILi7ELb1ELb0ELb0ELb1ELb1EEv7DParamsjj": (3, 168, 0, 168),
    "_Z11k_mutate_v5ILi8ELb0ELb1ELb0ELb0ELb0EEv7DParamsjj": (2, 191, 0, 191),
    "_Z11k_mutate_v5ILi8ELb0ELb1ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 92, 168),
    "_Z11k_mutate_v5ILi8ELb1ELb0ELb0ELb0ELb0EEv7DParamsjj": (2, 187, 0, 187),
    "_Z11k_mutate_v5ILi8ELb1ELb0ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 84, 168),
    "_Z11k_mutate_v5ILi8ELb1ELb0ELb1ELb0ELb0EEv7DParamsjj": (2, 219, 0, 219),
    "_Z11k_mutate_v5ILi8ELb1ELb1ELb0ELb0ELb0EEv7DParamsjj": (2, 197, 0, 197),
    "_Z11k_mutate_v5ILi8ELb1ELb1ELb0ELb0ELb1EEv7DParamsjj": (3, 168, 96, 168),
}


def _feat(name):
    return int(re.match(r"_Z11k_mutate_v\dILi(\d+)E", name).group(1)) & 15     # k_mutate_v4: BUILD = FEAT | 16 rule | 32 one light


def test_chain_kernels_keep_the_parents_occupancy_with_vertex_normals(native_lib):
    k = kernels(os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources"))
    now = {n: r for n, r in k.items() if re.match(r"_Z11k_mutate_v[345]", n)}
    assert sorted(now) == sorted(BUILDS)                 # no instantiation added, none lost
    for n, (occ, regs, scratch, pinned) in sorted(BUILDS.items()):
        r = now[n]
        mine = (r["Occupancy"], r["VGPRs"] + r["AGPRs"], r["ScratchSize"])
        if _feat(n) & 4:
            print("%s: occupancy %d (parent %d), registers %d (parent %d), scratch %d B (parent %d B)" % (n, mine[0], occ, mine[1], regs, mine[2], scratch))
            assert mine[0] >= occ and mine[1] <= pinned, (n, mine, (occ, regs, scratch, pinned))
        else:
            assert pinned == regs and mine == (occ, regs, scratch), (n, mine, (occ, regs, scratch))
