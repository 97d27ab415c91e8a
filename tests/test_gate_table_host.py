"""The gate table that the passes over many gate sequences share (csrc/ffk_api_gate_table.h), through every C entry
that takes one, on a machine without a GPU: a malformed table is FFK_EINVAL with one message whatever the entry, before
anything touches a device and with the outputs untouched; the workspace queries report what they reported before the
layouts shared their head; and the stand-alone program that drives the header under the host sanitizers builds and
runs clean."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from filter_functions_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, A = 7, 1

# (offsets, index) of three tables over T = 1 gate, and what the checker says of them
MALFORMED = [(([0, 2, 3], [0, 1, 0]), 'index[1] = 1 outside [0, 1)'),
             (([0, 2, 1], [0, 0, 0]), 'offsets not increasing at sequence 1 (2 -> 1)'),
             (([1, 2, 3], [0, 0, 0]), 'offsets[0] = 1, expected 0')]

ENTRIES = [('ffk_concatenate_sequences_resident', 2), ('ffk_sequence_correlation_infidelities', 2),
           ('ffk_sequence_correlation_infidelities4', 4), ('ffk_sequence_infidelities', 2),
           ('ffk_sequence_infidelities', 4), ('ffk_sequence_processes', 2), ('ffk_sequence_processes', 4),
           ('ffk_sequence_frequency_shifts', 2), ('ffk_sequence_frequency_shifts', 4)]


class Call:
    """One entry on a table of one gate without a handle; every output starts as NaN."""

    def __init__(self, name, d):
        rng = np.random.default_rng(d)
        N = d*d
        self.lib, self.name, self.d, self.N = _lib.load(), name, d, N
        self.gates = (ctypes.c_void_p*1)(None)
        self.slots = np.array([-1], dtype=np.int32)
        self.table = rng.normal(size=(1, A, N, W)) + 1j*rng.normal(size=(1, A, N, W))
        self.U = np.eye(d, dtype=np.complex128)[None].copy()
        self.tau = np.array([1.0])
        self.omega = np.linspace(0.1, 2.0, W)
        self.basis = rng.normal(size=(N, d, d)) + 0j
        self.S = np.ones(W)
        self.idx = np.zeros(1, dtype=np.int32)
        self.shifts = np.zeros((1, 1, 1, N, N))
        self.outputs = {k: np.full(shape, np.nan) for k, shape in dict(
            infid=(2, 1), total=(2, d, d, 2), F=(2, A, A, W, 2), ragged=(8, 1), tiles=(1, 2, 1, N, N)).items()}
        self.flags = np.full((1, 2), -7, dtype=np.int32)
        self.F_ptr = ctypes.c_void_p(0xBAD)

    def __call__(self, offsets, index):
        offsets, index = np.asarray(offsets, dtype=np.int32), np.asarray(index, dtype=np.int32)
        out = {k: v.ctypes.data for k, v in self.outputs.items()}
        head = (self.gates, self.slots.ctypes.data, self.table.ctypes.data, self.U.ctypes.data, self.tau.ctypes.data,
                1, offsets.ctypes.data, index.ctypes.data, len(offsets) - 1, self.omega.ctypes.data, W,
                self.basis.ctypes.data, 1, self.d, A, self.N)
        spectrum = (self.S.ctypes.data, 1, 1, self.idx.ctypes.data, 1, self.d)
        stacked = (self.S.ctypes.data, 1, 1, self.idx.ctypes.data, 1)
        entry = getattr(self.lib, self.name)
        if self.name == 'ffk_concatenate_sequences_resident':
            handle = ctypes.c_void_p()
            assert self.lib.ffk_resident_create(ctypes.byref(handle)) == 0
            try:
                return entry(handle, *head, *spectrum, out['total'], ctypes.byref(self.F_ptr), out['infid'])
            finally:
                assert self.lib.ffk_resident_destroy(handle) == 0
        if self.name.startswith('ffk_sequence_correlation_infidelities'):
            out_offsets = np.zeros(len(offsets), dtype=np.int64)
            np.cumsum(np.diff(offsets.astype(np.int64))**2, out=out_offsets[1:])
            return entry(*head, *spectrum, out_offsets.ctypes.data, out['ragged'])
        if self.name == 'ffk_sequence_infidelities':
            return entry(*head, *spectrum, out['infid'], out['total'], out['F'])
        if self.name == 'ffk_sequence_processes':
            return entry(*head, 0, *stacked, 1, out['tiles'], self.flags.ctypes.data, out['total'])
        return entry(*head, *stacked, self.shifts.ctypes.data, out['tiles'], self.flags.ctypes.data, out['total'])

    def untouched(self):
        return (all(np.isnan(v).all() for v in self.outputs.values()) and (self.flags == -7).all()
                and self.F_ptr.value == 0xBAD)


@pytest.mark.parametrize('name,d', ENTRIES)
def test_a_malformed_table_is_refused_by_every_entry(name, d):
    call = Call(name, d)
    for (offsets, index), message in MALFORMED:
        assert call(offsets, index) == _lib.FFK_EINVAL
        assert call.lib.ffk_last_error().decode() == message
        assert call.untouched()


# what the queries returned before the layouts shared the table's head; the arguments are (T, P, n_index, n_host, d, A,
# N, W, n_idx, s_ndim[, n_spectra[, stage]]); every entry with host rows, and with a cross-spectrum where it takes one
RECORDED = {
    ('ffk_concatenate_sequences_workspace_bytes', (3, 5, 40, 2, 2, 2, 4, 65, 2, 3)): 91136,
    ('ffk_concatenate_sequences_workspace_bytes', (24, 1050, 80850, 0, 2, 1, 4, 301, 1, 1)): 25821184,
    ('ffk_concatenate_sequences_workspace_bytes', (1, 1, 1, 1, 2, 4, 4, 7, 0, 0)): 8192,
    ('ffk_sequence_correlation_infidelities_workspace_bytes', (3, 5, 40, 2, 2, 2, 4, 65, 2, 2)): 187392,
    ('ffk_sequence_correlation_infidelities_workspace_bytes', (24, 7, 300, 0, 2, 1, 4, 301, 1, 1)): 12462592,
    ('ffk_sequence_correlation_infidelities4_workspace_bytes', (3, 5, 40, 3, 4, 2, 16, 65, 1, 2)): 279296,
    ('ffk_sequence_correlation_infidelities4_workspace_bytes', (25, 7, 300, 0, 4, 4, 16, 7, 4, 1)): 5599488,
    ('ffk_sequence_infidelities_workspace_bytes', (3, 5, 40, 2, 4, 2, 16, 65, 2, 3)): 110080,
    ('ffk_sequence_infidelities_workspace_bytes', (24, 1050, 80850, 0, 2, 1, 4, 301, 1, 1)): 5593856,
    ('ffk_sequence_infidelities_workspace_bytes', (5, 3, 9, 5, 2, 3, 4, 7, 0, 0)): 14080,
    ('ffk_sequence_processes_workspace_bytes', (3, 5, 40, 2, 4, 2, 16, 65, 2, 2, 3, 3)): 876544,
    ('ffk_sequence_processes_workspace_bytes', (3, 5, 40, 1, 2, 4, 4, 7, 3, 1, 2, 1)): 14080,
    ('ffk_sequence_processes_workspace_bytes', (25, 100, 5000, 0, 4, 1, 16, 301, 1, 1, 1, 2)): 3325696,
    ('ffk_sequence_frequency_shifts_workspace_bytes', (3, 5, 40, 2, 4, 2, 16, 65, 2, 2, 3)): 318464,
    ('ffk_sequence_frequency_shifts_workspace_bytes', (3, 5, 40, 3, 2, 4, 4, 7, 3, 1, 2)): 19712,
    ('ffk_sequence_frequency_shifts_workspace_bytes', (25, 100, 5000, 0, 4, 1, 16, 301, 1, 1, 1)): 1522176,
}


def test_the_workspace_queries_report_what_they_reported():
    lib = _lib.load()
    for (name, shape), nbytes in RECORDED.items():
        assert getattr(lib, name)(*shape) == nbytes, (name, shape)


def test_the_standalone_check_builds_and_runs_clean(tmp_path):
    """tools/check_gate_table.hip with the build line of its header comment: host code under ASan and UBSan, its own
    main, nothing preloaded."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    program = str(tmp_path/'check_gate_table')
    subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', '-Wno-unused-function', '-DFFK_HOST_SANITIZE',
                    '-Xarch_host', '-fsanitize=address,undefined', '-I' + os.path.join(ROOT, 'include'),
                    '-I' + os.path.join(ROOT, 'filter_functions_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'check_gate_table.hip'), '-o', program], check=True, cwd=ROOT)
    done = subprocess.run([program, '100', '3'], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == 'gate table: 100 rounds ok' and 'runtime error' not in done.stderr
