"""What the host tests of the C ABI share: reading include/vaek.h."""
import re


def _c_args(hdr, name):
    """Number of arguments include/vaek.h declares for the int function `name`."""
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/vaek.h"
    args = m.group(1).strip()
    return 0 if args == "void" else len(args.split(","))


def check_description_guard(lib, name):
    """Entry point `name` (its third argument the description) with a NULL context: a NULL description and a struct_size eight bytes
    short are refused with the entry's name, the latter with both sizes, before the context is looked at; the right size reaches the
    context check.  Nothing needs a device."""
    import ctypes as C

    from vae_training_amd import _lib
    argtypes = _lib.SIGNATURES[name][1]
    mirror = argtypes[2]._type_
    rest = [None if t is C.c_void_p else 0 for t in argtypes[3:]]
    who = name.encode()
    assert getattr(lib, name)(None, None, None, *rest) == -1
    assert lib.vaek_last_error().startswith(who + b": ") and b"description" in lib.vaek_last_error(), lib.vaek_last_error()
    desc = mirror()
    want = C.sizeof(mirror)
    desc.struct_size = want - 8
    assert getattr(lib, name)(None, None, C.byref(desc), *rest) == -1
    err = lib.vaek_last_error()
    assert err.startswith(who + b": ") and b"struct_size %d != %d" % (want - 8, want) in err, err
    desc.struct_size = want
    assert getattr(lib, name)(None, None, C.byref(desc), *rest) == -1
    err = lib.vaek_last_error()
    assert err.startswith(who + b": ") and b"null context" in err, err
