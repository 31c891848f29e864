"""Host side of the training entry points that take a description, no GPU: each checks its vaek_replicas, and the traced ones their
vaek_trajectory, before its context (the order is in csrc/eval_check.h)."""
import ctypes as C

import pytest

from tests.abi_util import check_description_guard, sized

REPLICA_ENTRIES = ("vaek_train_loop_gen_replicas", "vaek_train_loop_gen_replicas_traj", "vaek_train_step_gen_replicas")
TRACED_ENTRIES = ("vaek_train_loop_gen_traj", "vaek_train_loop_gen_replicas_traj")


@pytest.mark.parametrize("name", REPLICA_ENTRIES)
def test_the_description_is_checked_before_the_context(name):
    """With a NULL context: a NULL rep gives -1 and the entry's name; a struct_size eight bytes short gives -1, the name and
    `struct_size <got> != <want>` with <want> the ctypes mirror's size; the right size gives -1 and "null context"."""
    from vae_training_amd import _lib
    check_description_guard(_lib.load(), name, index=6)


@pytest.mark.parametrize("name", TRACED_ENTRIES)
def test_the_trajectory_size_is_checked_before_the_context(name):
    """With a NULL context and, where the entry takes one, a vaek_replicas of the right size: a vaek_trajectory eight bytes short is
    refused with the entry's name and both sizes; one of the right size reaches "null context"; a NULL traj stays the plain call and
    answers in the untraced entry's name."""
    from vae_training_amd import _lib
    lib = _lib.load()
    argtypes = _lib.SIGNATURES[name][1]
    rep = sized(_lib.VaekReplicas)
    head = [C.byref(rep) if t is C.POINTER(_lib.VaekReplicas) else None if t is C.c_void_p else 0 for t in argtypes[:-1]]
    want = C.sizeof(_lib.VaekTrajectory)
    assert getattr(lib, name)(*head, C.byref(sized(_lib.VaekTrajectory, 8))) == -1
    err = lib.vaek_last_error()
    assert err.startswith(name.encode() + b": ") and b"vaek_trajectory.struct_size %d != %d" % (want - 8, want) in err, err
    assert getattr(lib, name)(*head, C.byref(sized(_lib.VaekTrajectory))) == -1
    err = lib.vaek_last_error()
    assert err.startswith(name.encode() + b": ") and b"null context" in err, err
    assert getattr(lib, name)(*head, None) == -1
    err = lib.vaek_last_error()
    assert err.startswith(name[:-len("_traj")].encode() + b": ") and b"null context" in err, err
