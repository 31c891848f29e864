"""What the host tests of the C ABI share: reading include/vaek.h."""
import re


def _c_args(hdr, name):
    """Number of arguments include/vaek.h declares for the int function `name`."""
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/vaek.h"
    args = m.group(1).strip()
    return 0 if args == "void" else len(args.split(","))


def sized(mirror, short=0):
    """An instance of the ctypes mirror of a struct_size-guarded struct, its struct_size `short` bytes below the mirror's size."""
    import ctypes as C
    d = mirror()
    d.struct_size = C.sizeof(mirror) - short
    return d


def check_description_guard(lib, name, index=2):
    """Entry point `name` (argument `index` the description) with a NULL context: a NULL description and a struct_size eight bytes
    short are refused with the entry's name, the latter with both sizes, before the context is looked at; the right size reaches the
    context check.  Every other pointer is NULL, every number 0, and a further struct_size-guarded struct behind the description is
    given at its right size (the traced training calls answer in their own name only with a trajectory).  Nothing needs a device."""
    import ctypes as C

    from vae_training_amd import _lib
    argtypes = _lib.SIGNATURES[name][1]
    mirror = argtypes[index]._type_
    guarded = lambda t: hasattr(getattr(t, "_type_", None), "struct_size")          # a pointer to a struct_size-guarded struct
    rest = [None if t is C.c_void_p else C.pointer(sized(t._type_)) if guarded(t) else 0 for t in argtypes[index + 1:]]
    call = lambda desc: getattr(lib, name)(*[None] * index, desc, *rest)
    who = name.encode()
    assert call(None) == -1
    assert lib.vaek_last_error().startswith(who + b": ") and b"description" in lib.vaek_last_error(), lib.vaek_last_error()
    want = C.sizeof(mirror)
    assert call(C.byref(sized(mirror, 8))) == -1
    err = lib.vaek_last_error()
    assert err.startswith(who + b": ") and b"struct_size %d != %d" % (want - 8, want) in err, err
    assert call(C.byref(sized(mirror))) == -1
    err = lib.vaek_last_error()
    assert err.startswith(who + b": ") and b"null context" in err, err
