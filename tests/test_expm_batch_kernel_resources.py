"""The two kernels of the batched exponential (expm_batch.hip, ffk_expm_real_batch) keep nothing in private memory and
spill no register -- read from libffk.so as test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

EXPM_BATCH = ('expm_batch_lane4_kernel', 'expm_batch_wave_kernel')


@pytest.mark.parametrize('fragment', EXPM_BATCH)
def test_expm_batch_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert len(found) == 1, (fragment, sorted(found))
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name


def test_the_lane_kernel_uses_no_lds_and_the_wave_kernel_no_tile(kernels):  # noqa: F811
    """One matrix per lane lives in registers alone.  One matrix per wavefront keeps its tiles in registers as well:
    what LDS it is charged is the scratch of the cross-lane steps of the norm at most, never a 16 x 17 tile (2176
    bytes) per wavefront."""
    lane = [k for name, k in kernels.items() if EXPM_BATCH[0] in name][0]
    wave = [k for name, k in kernels.items() if EXPM_BATCH[1] in name][0]
    assert lane['.group_segment_fixed_size'] == 0
    assert wave['.group_segment_fixed_size'] < 2176
    # a block of four wavefronts, one per SIMD: each within the 512 registers of a SIMD lane
    assert lane['.vgpr_count'] <= 512 and wave['.vgpr_count'] <= 128
