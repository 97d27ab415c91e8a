"""The kernels of the batched pulse-correlation infidelities (correlations.hip) keep nothing in private memory, spill
no register and fit the register file at their block size -- read from libffk.so as test_kernel_resources.py does (CPU
test)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)


def _check(name, k):
    assert k['.private_segment_fixed_size'] == 0, name
    assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
    assert k['.max_flat_workgroup_size'] == 256, name
    # 256 threads are four wavefronts, one per SIMD: the whole file of 512 registers
    waves_per_simd = k['.max_flat_workgroup_size']//64//4
    # (gfx950 has one unified file: the metadata's .vgpr_count is the total, the accumulation registers included)
    assert k['.vgpr_count'] >= k.get('.agpr_count', 0)
    assert k['.vgpr_count'] <= 512//waves_per_simd, (name, k['.vgpr_count'], k.get('.agpr_count'))


def test_the_gram_kernel_has_one_instantiation_per_length_class(kernels):  # noqa: F811
    found = {name: k for name, k in kernels.items() if 'correlation_gram_kernel' in name}
    assert len(found) == 4, sorted(found)
    for c in range(4):
        assert sum(f'ILi{c}E' in name for name in found) == 1, (c, sorted(found))
    for name, k in found.items():
        _check(name, k)
        assert k['.group_segment_fixed_size'] == 0, name       # (its LDS is sized at the launch)


@pytest.mark.parametrize('fragment', ['correlation_prefix_kernel', 'correlation_reduce_kernel'])
def test_the_small_kernels(kernels, fragment):  # noqa: F811
    found = {name: k for name, k in kernels.items() if fragment in name}
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        _check(name, k)
