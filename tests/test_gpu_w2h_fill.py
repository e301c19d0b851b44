"""k_mutate_w2h (k_mutate_w2<true>, kernels_v4.hip) fills the proposal rows of the chains it has decided in ONE flattened pass: the
first-stage and coin items of the chains that start a mutation, and behind them the second-stage items of the chains whose first
stage was rejected, one PAIR of a Philox block each, all drawn at one Philox site; a second-stage item's tail is
row_fill_second_pair_drawn (device_sampler.h). k_mutate_w2 and k_mutate_v4's twin keep the two loops and RowSamplerT::fill_second.

Three contexts run the same chains BIT FOR BIT -- states, f(u) of the current states, every counter of stats(): the default one,
one under DRMLT_NO_W2_HELD=1 and one under DRMLT_NO_W2=1 (tests/test_gpu_w2h.py: three, check; films to the reordering bound of
tests/test_gpu_w2.py). Each run must be eventful (second stages, large steps, accepted and rejected mutations).

The cases are the shapes at which the merged pass takes another path (n1 / n2: chains of a call that start a mutation / a second
stage; a first-stage chain has nb1 + 1 = D4/4 + 1 items, a second-stage chain 4 nb2):
  DRMLT_MH_BATCH=1    a call decides one chain: a pass holds one chain's first-stage and coin items (n2 == 0) or one chain's
                      second-stage items alone (n1 == 0)
  DRMLT_MH_BATCH=32   10 n1 + 20 n2 crosses 192 and 256: a fourth and a fifth trip, the second-stage items spread over several
  timid_after_large   the uniform arm: nb2 = D4/4, a rejected large step stores four uniforms through pairs 0 and 1, a bold
                      one's blocks beyond its own count store nothing
  max_depth 2 and 3   6 and 10 dimensions: D4/2 = 4 fills the last block's four pairs, D4/2 = 6 only two of them -- the stores
                      of the other two would land in the next row group
  80 chains, sliced   a half-empty last wave over two calls in launches of 16 mutations"""
import pytest

from test_gpu_w2 import N_CHAINS, N_MUT
from test_gpu_w2h import check, three

pytestmark = pytest.mark.gpu


def same_and_eventful(h, s, t, waves, mutations):
    st = h["stats"]
    print("second_base", st.second_base, "large_base", st.large_base, "bold_base", st.bold_base, "first", st.first_acc, st.first_base, "accepted", st.accepted)
    check(h, s, t, waves, mutations)  # (assert_eventful, then assert_same against the twin for both w2 builds)


@pytest.mark.parametrize("batch", [1, 32])
def test_batches(pkg, native_lib, capfd, batch):
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], env={"DRMLT_MH_BATCH": str(batch)})
    same_and_eventful(h, s, t, 3, N_CHAINS * N_MUT)


def test_uniform_arm(pkg, native_lib, capfd):
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], timid_after_large=1)
    print("second_large_base", h["stats"].second_large_base)
    assert h["stats"].second_large_base > 0
    same_and_eventful(h, s, t, 3, N_CHAINS * N_MUT)


@pytest.mark.parametrize("max_depth", [2, 3], ids=["last_block_full", "last_block_half_masked"])
def test_last_block(pkg, native_lib, capfd, max_depth):
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], max_depth=max_depth)
    same_and_eventful(h, s, t, 3, N_CHAINS * N_MUT)


def test_half_empty_last_wave_sliced(pkg, native_lib, capfd):
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT // 2, N_MUT // 2], env={"DRMLT_SLICE": "16"}, n_chains=80)
    same_and_eventful(h, s, t, 12, 80 * N_MUT)
