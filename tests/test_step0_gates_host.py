"""CPU: the with-gates prepare entries (the typed encoder's step-0 gate table behind the message table) size their buffer
as documented and refuse bad arguments before any device call - the library loads without a GPU, as in test_cabi.py."""
from ionic_mpnn_amd import _lib

F32, F16X2, TYPED, X3 = 0, 1, 2, 3
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
P = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first


def _old(lib, D, S, Vb, mode):
    return int(lib.impnn_encoder_prepared_bytes(D, S, Vb, mode))


def _atoms(lib, D, S, Va, Vb, mode):
    return int(lib.impnn_encoder_prepared_bytes_atoms(D, S, Va, Vb, mode))


def _gates(lib, D, S, Va, Vb, mode):
    return int(lib.impnn_encoder_prepared_bytes_gates(D, S, Va, Vb, mode))


def _round16(n):
    return (n + 15) // 16 * 16


def test_size_is_the_with_atoms_size_plus_the_gate_table():
    lib = _lib.load()
    for mode in (TYPED, X3):
        for S, Va, Vb in [(3, 124, 72), (1, 5, 3), (4, 1500, 3), (3, 63, 256), (3, 1, 1), (3, 255, 64)]:
            assert Vb * (Va + 1) * 128 <= 2 << 20
            assert _gates(lib, 32, S, Va, Vb, mode) == _round16(_atoms(lib, 32, S, Va, Vb, mode) + (Va + 1) * 256)
    assert _gates(lib, 32, 3, 124, 72, X3) == _old(lib, 32, 3, 72, X3) + 72 * 125 * 128 + 125 * 256


def test_the_with_atoms_entries_keep_their_sizes():
    lib = _lib.load()
    for mode in (TYPED, X3):
        assert _atoms(lib, 32, 3, 124, 72, mode) == _old(lib, 32, 3, 72, mode) + 72 * 125 * 128


def test_size_is_the_old_one_where_the_message_table_is_refused():
    lib = _lib.load()
    for mode in (TYPED, X3):
        assert _gates(lib, 32, 3, 300, 72, mode) == _old(lib, 32, 3, 72, mode) > 0  # beyond the 2 MiB cap
        assert _gates(lib, 32, 3, 256, 64, mode) == _old(lib, 32, 3, 64, mode) > 0  # one column beyond it
        assert _gates(lib, 32, 0, 124, 72, mode) == _old(lib, 32, 0, 72, mode)      # no step
    for mode in (F32, F16X2):                                                       # pull modes
        assert _gates(lib, 32, 3, 124, 72, mode) == _old(lib, 32, 3, 72, mode) > 0
    for D in (64, 128):                                                             # wide states
        assert _gates(lib, D, 3, 124, 72, TYPED) == _old(lib, D, 3, 72, TYPED) > 0
    assert _gates(lib, 48, 3, 124, 72, TYPED) == 0 and _gates(lib, 32, 3, 124, 72, 4) == 0
    assert _gates(lib, 32, 3, 0, 72, TYPED) == 0 and _gates(lib, 32, 3, -1, 72, TYPED) == 0


def _prepare(lib, weights=P, bond=P, atoms=P, Va=124, D=32, K=8, S=3, Vb=72, mode=TYPED, out=P, nbytes=None):
    if nbytes is None:
        nbytes = _gates(lib, D, S, Va, Vb, mode)
    return lib.impnn_encoder_prepare_weights_gates(weights, bond, atoms, Va, D, K, S, Vb, mode, out, nbytes, None)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    for mode in (TYPED, X3):
        assert _prepare(lib, weights=None, mode=mode) == BADARG and b"null" in lib.impnn_last_error_string()
        assert _prepare(lib, bond=None, mode=mode) == BADARG
        assert _prepare(lib, atoms=None, mode=mode) == BADARG
        assert _prepare(lib, out=None, mode=mode) == BADARG
        assert _prepare(lib, out=P + 8, mode=mode) == BADARG and b"aligned" in lib.impnn_last_error_string()
        assert _prepare(lib, atoms=P + 4, mode=mode) == BADARG and b"aligned" in lib.impnn_last_error_string()
        need = _gates(lib, 32, 3, 124, 72, mode)
        assert _prepare(lib, mode=mode, nbytes=need - 1) == WORKSPACE
        # the with-atoms size and the plain image's are too small once a gate table follows
        assert _prepare(lib, mode=mode, nbytes=_atoms(lib, 32, 3, 124, 72, mode)) == WORKSPACE
        assert _prepare(lib, mode=mode, nbytes=_old(lib, 32, 3, 72, mode)) == WORKSPACE
        assert b"bytes" in lib.impnn_last_error_string()
        assert _prepare(lib, mode=mode, Va=300, nbytes=_old(lib, 32, 3, 72, mode) - 1) == WORKSPACE  # beyond the cap
    assert _prepare(lib, Va=0) == BADARG and _prepare(lib, Va=-5) == BADARG
    assert _prepare(lib, Vb=0) == BADARG and _prepare(lib, K=0) == BADARG and _prepare(lib, S=-1) == BADARG
    assert _prepare(lib, mode=4) == BADARG and _prepare(lib, mode=-1) == BADARG
    assert _prepare(lib, D=48, nbytes=1 << 20) == UNSUPPORTED
    assert _prepare(lib, Vb=257, nbytes=1 << 30) == UNSUPPORTED
    assert _prepare(lib, atoms=None, mode=F32) == BADARG  # the table is an argument of the entry in every mode
    assert _prepare(lib, S=0, weights=None, out=None, nbytes=0) == 0  # nothing to build
