"""filter_functions_amd -- the numeric hot path of qutech/filter_functions on AMD MI355X.

A drop-in for ``PulseSequence.get_filter_function()`` and ``ff.infidelity()``::

    import filter_functions_amd as ff

    pulse = ff.PulseSequence(H_c, H_n, dt, basis=ff.Basis.pauli(2))
    F = pulse.get_filter_function(omega)
    infid = ff.infidelity(pulse, spectrum, omega)

The arithmetic runs in hand-written HIP kernels for gfx950 behind a C ABI
(``include/ffk.h``, ``filter_functions_amd/libffk.so``); this package is the Python host
side: the reference's object model, argument checking, caching and exceptions.
See DESIGN.md for the scope, INTEGRATION.md for the boundary.
"""
from . import (analytic, basis, batch, batch_gradient, batch_second_order, correlations, expm_batch, gradient, numeric, periodic, periodic_second_order, processes, pulse_sequence, sequences,
               sequence_gradient, sequence_prefix_second_order, sequence_prefixes, sequence_processes, sequence_second_order,
               superoperator, util)
from .basis import Basis
from .batch import get_filter_functions, infidelities
from .batch_gradient import filter_function_derivatives, infidelity_derivatives
from .batch_second_order import frequency_shifts
from .correlations import correlation_infidelities
from .expm_batch import exponentiate_cumulant_functions
from .gradient import infidelity_derivative
from .numeric import error_transfer_matrix, infidelity
from .periodic import periodic_decay_amplitudes, periodic_filter_functions, periodic_infidelities
from .periodic_second_order import (periodic_cumulant_functions, periodic_error_transfer_matrices,
                                    periodic_frequency_shifts)
from .processes import cumulant_functions, decay_amplitudes, error_transfer_matrices
from .sequences import concatenate_sequences
from .sequence_correlations import sequence_correlation_infidelities
from .sequence_gradient import (gate_infidelity_derivatives, sequence_filter_function_derivatives,
                                sequence_infidelity_derivatives)
from .sequence_infidelities import sequence_infidelities
from .sequence_prefixes import (sequence_prefix_decay_amplitudes, sequence_prefix_infidelities,
                                sequence_prefix_propagators)
from .sequence_prefix_second_order import (sequence_prefix_cumulant_functions, sequence_prefix_error_transfer_matrices,
                                           sequence_prefix_frequency_shifts)
from .sequence_processes import (sequence_cumulant_functions, sequence_decay_amplitudes,
                                 sequence_error_transfer_matrices)
from .sequence_second_order import sequence_frequency_shifts
from .pulse_sequence import (PulseSequence, concatenate, concatenate_periodic,
                             concatenate_without_filter_function, extend, remap)
from .superoperator import liouville_representation

__all__ = ['analytic', 'Basis', 'PulseSequence', 'basis', 'batch', 'batch_gradient', 'batch_second_order',
           'concatenate',
           'concatenate_periodic',
           'concatenate_sequences',
           'correlation_infidelities', 'correlations',
           'concatenate_without_filter_function', 'cumulant_functions', 'decay_amplitudes',
           'error_transfer_matrices', 'error_transfer_matrix', 'expm_batch', 'exponentiate_cumulant_functions', 'extend', 'get_filter_functions', 'gradient', 'infidelities', 'infidelity',
           'filter_function_derivatives', 'frequency_shifts', 'gate_infidelity_derivatives', 'infidelity_derivative', 'infidelity_derivatives',
           'liouville_representation', 'numeric', 'periodic', 'periodic_decay_amplitudes',
           'periodic_cumulant_functions', 'periodic_error_transfer_matrices', 'periodic_filter_functions',
           'periodic_frequency_shifts', 'periodic_infidelities', 'periodic_second_order', 'processes',
           'pulse_sequence', 'remap', 'sequence_correlation_infidelities', 'sequence_correlations',
           'sequence_cumulant_functions', 'sequence_decay_amplitudes',
           'sequence_error_transfer_matrices', 'sequence_filter_function_derivatives', 'sequence_frequency_shifts',
           'sequence_gradient', 'sequence_infidelities', 'sequence_infidelity_derivatives',
           'sequence_prefix_cumulant_functions', 'sequence_prefix_decay_amplitudes',
           'sequence_prefix_error_transfer_matrices', 'sequence_prefix_frequency_shifts',
           'sequence_prefix_infidelities', 'sequence_prefix_propagators', 'sequence_prefix_second_order',
           'sequence_prefixes', 'sequence_processes',
           'sequence_second_order', 'sequences',
           'superoperator', 'util']

__version__ = '0.1.0'
