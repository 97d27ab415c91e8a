"""The kernels of the batched frequency shifts (second.hip, ffk_batch_frequency_shifts) keep nothing in private memory
and spill no register -- read from libffk.so as test_kernel_resources.py does (CPU test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)

SMALL = ('so_prepare_pulses_kernel', 'so_shift_reduce_kernel', 'prologue_pulses_kernel')


def test_the_fused_kernel_has_two_instantiations_without_private_memory(kernels):  # noqa: F811
    """so_shift_kernel<MT, MT> for MT = 1, 2: the accumulators of one frequency (8 MT^2 doubles per lane) and the
    weighted real sums (4 MT^2) stay in registers at two wavefronts per SIMD."""
    found = {name: k for name, k in kernels.items() if 'so_shift_kernel' in name}
    assert len(found) == 2, sorted(found)
    for MT in (1, 2):
        assert sum(f'ILi{MT}ELi{MT}E' in name for name in found) == 1, (MT, sorted(found))
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] == 256, name
        assert k['.vgpr_count'] + k['.agpr_count'] <= 256, (name, k['.vgpr_count'], k['.agpr_count'])


@pytest.mark.parametrize('fragment', SMALL)
def test_the_small_kernels_keep_nothing_in_private_memory(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name and 'apply_' not in name}
    assert found, fragment
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] <= 256, name
