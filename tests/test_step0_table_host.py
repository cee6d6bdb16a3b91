"""CPU: the with-atoms prepare entries (the typed encoder's step-0 message table) size their buffer as documented and
refuse bad arguments before any device call - the library loads without a GPU, as in test_cabi.py."""
import ctypes as C

from ionic_mpnn_amd import _lib

F32, F16X2, TYPED, X3 = 0, 1, 2, 3
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
P = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first


def _old(lib, D, S, Vb, mode):
    return int(lib.impnn_encoder_prepared_bytes(D, S, Vb, mode))


def _new(lib, D, S, Va, Vb, mode):
    return int(lib.impnn_encoder_prepared_bytes_atoms(D, S, Va, Vb, mode))


def test_abi_version_is_unchanged():
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_size_is_the_old_image_plus_the_table_under_the_cap():
    lib = _lib.load()
    for mode in (TYPED, X3):
        for S, Va, Vb in [(3, 124, 72), (1, 5, 3), (4, 1500, 3), (3, 63, 256), (3, 1, 1)]:
            assert Vb * (Va + 1) * 128 <= 2 << 20
            assert _new(lib, 32, S, Va, Vb, mode) == _old(lib, 32, S, Vb, mode) + Vb * (Va + 1) * 128
    # exactly at the cap, and one column beyond it
    assert _new(lib, 32, 3, 255, 64, TYPED) == _old(lib, 32, 3, 64, TYPED) + (2 << 20)
    assert _new(lib, 32, 3, 256, 64, TYPED) == _old(lib, 32, 3, 64, TYPED)


def test_size_is_the_old_one_where_no_table_is_built():
    lib = _lib.load()
    assert _new(lib, 32, 3, 300, 72, TYPED) == _old(lib, 32, 3, 72, TYPED) > 0      # beyond the cap
    assert _new(lib, 32, 3, 300, 72, X3) == _old(lib, 32, 3, 72, X3) > 0
    assert _new(lib, 32, 0, 124, 72, TYPED) == _old(lib, 32, 0, 72, TYPED)          # no step, no step-0 messages
    for mode in (F32, F16X2):                                                       # pull modes
        assert _new(lib, 32, 3, 124, 72, mode) == _old(lib, 32, 3, 72, mode) > 0
    for D in (64, 128):                                                             # wide states
        assert _new(lib, D, 3, 124, 72, TYPED) == _old(lib, D, 3, 72, TYPED) > 0
    assert _new(lib, 48, 3, 124, 72, TYPED) == 0 and _new(lib, 32, 3, 124, 72, 4) == 0
    assert _new(lib, 32, 3, 0, 72, TYPED) == 0 and _new(lib, 32, 3, -1, 72, TYPED) == 0


def test_the_old_entries_keep_their_results():
    lib = _lib.load()
    assert _old(lib, 32, 3, 72, TYPED) == (3 * 8192 + 3 * 72 * 1024 + 72 * 1024) * 4
    assert _old(lib, 32, 3, 72, X3) == (3 * 12288 + 3 * 72 * 1024 + 72 * 1024) * 4


def _prepare(lib, weights=P, bond=P, atoms=P, Va=124, D=32, K=8, S=3, Vb=72, mode=TYPED, out=P, nbytes=None):
    if nbytes is None:
        nbytes = _new(lib, D, S, Va, Vb, mode)
    return lib.impnn_encoder_prepare_weights_atoms(weights, bond, atoms, Va, D, K, S, Vb, mode, out, nbytes, None)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    for mode in (TYPED, X3):
        assert _prepare(lib, weights=None, mode=mode) == BADARG and b"null" in lib.impnn_last_error_string()
        assert _prepare(lib, bond=None, mode=mode) == BADARG
        assert _prepare(lib, atoms=None, mode=mode) == BADARG
        assert _prepare(lib, out=None, mode=mode) == BADARG
        assert _prepare(lib, out=P + 8, mode=mode) == BADARG and b"aligned" in lib.impnn_last_error_string()
        assert _prepare(lib, atoms=P + 4, mode=mode) == BADARG and b"aligned" in lib.impnn_last_error_string()
        need = _new(lib, 32, 3, 124, 72, mode)
        assert _prepare(lib, mode=mode, nbytes=need - 1) == WORKSPACE
        # the old image's size is too small once a table follows it
        assert _prepare(lib, mode=mode, nbytes=_old(lib, 32, 3, 72, mode)) == WORKSPACE
        assert b"bytes" in lib.impnn_last_error_string()
    assert _prepare(lib, Va=0) == BADARG and _prepare(lib, Va=-5) == BADARG
    assert _prepare(lib, Vb=0) == BADARG and _prepare(lib, K=0) == BADARG and _prepare(lib, S=-1) == BADARG
    assert _prepare(lib, mode=4) == BADARG and _prepare(lib, mode=-1) == BADARG
    assert _prepare(lib, D=48, nbytes=1 << 20) == UNSUPPORTED
    assert _prepare(lib, Vb=257, nbytes=1 << 30) == UNSUPPORTED
    assert _prepare(lib, atoms=None, mode=F32) == BADARG  # the table is an argument of the entry in every mode
    assert _prepare(lib, S=0, weights=None, out=None, nbytes=0) == 0  # nothing to build
