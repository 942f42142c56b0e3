"""The ICU library of the image (libicuuc), the second source of the Unicode tests (tests/test_unicode_second_source.py, tests/test_filter_model.py)."""
import ctypes as C


def load_icu():
    """(library, symbol suffix) — ICU's exports carry its major version, e.g. u_toupper_70 — or (None, None) when no ICU library loads."""
    for name in ("libicuuc.so.70", "libicuuc.so"):
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        for suffix in ("_70", ""):
            if hasattr(lib, "u_tolower" + suffix):
                return lib, suffix
    return None, None
