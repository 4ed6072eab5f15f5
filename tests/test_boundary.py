"""The one C-boundary guard of the library (holoagent_amd/csrc/hmsg_boundary.h): what each kind of exception becomes as a
(status, message) pair, on the product library itself.  The hook throws inside the guard and returns what the guard made of it;
no device is opened and nothing is launched."""
import ctypes as C

import pytest

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_NOMEM = 0, -1, -3, -4


@pytest.fixture(scope="module")
def L():
    from holoagent_amd._lib import HmsgLib
    return HmsgLib()


@pytest.mark.parametrize("kind,status,message", [
    (0, OK, ""),                                   # returns normally
    (1, ERR_UNSUPPORTED, "x"),                     # the library's own error keeps its code and message
    (2, ERR_NOMEM, "out of host memory"),          # std::bad_alloc
    (3, ERR_INVALID, "y"),                         # any other std::exception (std::length_error): its what()
    (4, ERR_INVALID, "unknown error"),             # anything else (an int)
])
def test_boundary_maps_exceptions(L, kind, status, message):
    msg = C.create_string_buffer(b"\xff" * 63, 64)
    assert L.c.hmsg_test_boundary(kind, msg, len(msg)) == status
    assert msg.value.decode() == message
    # the process is alive and the library still answers
    assert L.c.hmsg_test_boundary(0, msg, len(msg)) == OK
    assert msg.value == b""
