"""Every keyed entry point leaves no expanded key schedule behind (no GPU needed).

A call expands its key into a schedule on its own stack; the schedule is declared so that every way out of the function
wipes it (KEYSCHED, csrc/uaes_engine.h).  uaes_debug_live_key_schedules() counts schedules expanded and not yet wiped,
so after any call -- whatever it returned -- the count is what it was before.  Two kinds of call per keyed export
(tests/key_wipe_cases.py):

 (a) one that gets past the key expansion (where the function has one before its argument checks) and then fails an
     argument check before any device is touched;
 (b) with the host data path switched on, one successful call at 16 and at 17 bytes where the mode has a host path
     and takes the length, and one forged input for each authenticating decryption.

The list of keyed exports comes from include/uaes_hip.h: a new export without a case fails the test.  With nothing but
the counter added to the code as it was before, 44 of the (a) cases and the host-path cases of GCM-SIV and
uaes_cbc_decrypt_blocks fail on the count (the return codes are the same): the GPU-path modes wiped on the host path
only, and never on an argument error."""
import re

import pytest

import micro_aes_amd as uaes
from tests.key_wipe_cases import ARG_CASES, TEXT_CASES, HostMem, checked, keyed_exports


def test_every_keyed_export_has_a_case():
    names = keyed_exports()
    assert len(names) >= 90 and sorted(ARG_CASES) == names


@pytest.mark.parametrize("name", sorted(ARG_CASES))
def test_argument_error_behind_the_key_expansion_leaves_no_schedule(name):
    args, want = ARG_CASES[name]
    checked(name, args, want)


@pytest.fixture()
def host_forced():
    prev = uaes.host_policy(1 << 62, 1, 1)
    yield
    uaes.host_policy(*prev)


@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("case", range(len(TEXT_CASES)))
def test_host_path_call_leaves_no_schedule(host_forced, case, n):
    ran = 0
    for name, args, want in TEXT_CASES[case](n, HostMem):
        checked(name, args, want)
        ran += 1
    assert ran


# ---- key wrap with padding by name: its calls came into the lists last, from a module of their own that is gone, and
# these say so in the ids whatever position the lists give them
KWP_TEXT = next(c for c in TEXT_CASES if next(c(16, HostMem))[0] == "uaes_kwp_wrap")


def test_the_lists_hold_the_kwp_calls():
    names = {n for n in keyed_exports() if n.startswith("uaes_kwp_")}
    assert len(names) == 4 and names <= set(ARG_CASES)
    assert {name for name, _, _ in KWP_TEXT(17, HostMem)} == {n for n in names if not n.endswith("_batch")}


@pytest.mark.parametrize("name", ["uaes_kwp_unwrap", "uaes_kwp_unwrap_batch", "uaes_kwp_wrap", "uaes_kwp_wrap_batch"])
def test_kwp_argument_error_leaves_no_schedule(name):
    args, want = ARG_CASES[name]
    assert want == (1 if name in ("uaes_kwp_wrap", "uaes_kwp_unwrap") else -2)      # a length; a NULL array
    checked(name, args, want)


@pytest.mark.parametrize("n", [16, 17])
def test_kwp_host_path_wraps_unwraps_and_refuses_a_forgery(host_forced, n):
    """16 bytes: whole semiblocks; 17: seven fill bytes"""
    ran = []
    for name, args, want in KWP_TEXT(n, HostMem):
        checked(name, args, want)
        ran.append((name, want))
    assert ran == [("uaes_kwp_wrap", 0), ("uaes_kwp_unwrap", 0), ("uaes_kwp_unwrap", 0x1A)]


def test_host_cases_reach_every_export_with_a_host_path(host_forced):
    reached = set()
    for case in TEXT_CASES:
        for name, args, want in case(16, HostMem):
            checked(name, args, want)              # (a decryption's input has to exist)
            reached.add(name)
    # the batch, record, key-context, stream, multi-GPU and *_dev calls have no host path
    without = {n for n in keyed_exports() if re.search(r"_batch$|_dev$|^uaes_mgpu_|^uaes_gcm_(stream|key)_|^uaes_expand_key$", n)}
    assert reached == set(keyed_exports()) - without
