"""The kernels of the two-qubit pulse-correlation infidelities (correlations_d4.hip) keep nothing in private memory,
spill no register and fit the register file at their block size -- read from libffk.so as test_kernel_resources.py
does (CPU test)."""
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)


def _check(name, k):
    assert k['.private_segment_fixed_size'] == 0, name
    assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
    assert k['.max_flat_workgroup_size'] == 256, name
    # 256 threads are four wavefronts, one per SIMD: the whole file of 512 registers (the metadata's .vgpr_count is
    # the total of the unified file, the accumulation registers included)
    assert k['.vgpr_count'] >= k.get('.agpr_count', 0)
    assert k['.vgpr_count'] <= 512, (name, k['.vgpr_count'], k.get('.agpr_count'))


def test_the_gram_kernel_has_one_instantiation_per_length_class(kernels):  # noqa: F811
    found = {name: k for name, k in kernels.items() if 'correlations4_gram_kernel' in name}
    assert len(found) == 4, sorted(found)
    for c in range(4):
        assert sum(f'ILi{c}E' in name for name in found) == 1, (c, sorted(found))
    for name, k in found.items():
        _check(name, k)
        assert k['.group_segment_fixed_size'] == 0, name       # (its LDS is sized at the launch)


def test_the_prefix_kernel(kernels):  # noqa: F811
    found = {name: k for name, k in kernels.items() if 'correlations4_prefix_kernel' in name}
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        _check(name, k)
        assert k['.group_segment_fixed_size'] == 2*256*8, name      # two buffers of the 16 x 16 product


def test_the_single_qubit_kernels_gained_no_instantiation(kernels):  # noqa: F811
    for fragment, count in (('correlation_gram_kernel', 4), ('correlation_prefix_kernel', 1),
                            ('correlation_reduce_kernel', 1)):
        assert sum(fragment in name for name in kernels) == count, fragment
