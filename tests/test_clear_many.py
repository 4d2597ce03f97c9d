"""lvsr_clear_many: byte ranges of any address and length zeroed in one launch, nothing outside them touched.  The body runs on the CPU
emulator (same sources) and, under the `gpu` marker, on the device."""
import pytest
import torch

from emu import emu_lib

GUARD = 64              # bytes of pattern kept in front of and behind every range
PATTERN = 0xA5
MAX_MEMBERS = 64        # CLEAR_MANY_MAX of csrc/gemm.hip: one launch takes that many ranges

# bytes: 1, 3, 4, 5, 1 023 and 2^20 + 5 floats, and lengths that are no multiple of 4 (shorter than one 16-byte piece, and longer)
SIZES = [4, 12, 16, 20, 4092, ((1 << 20) + 5) * 4, 1, 7, 18, 4093]
# where a range starts relative to a 16-byte boundary: on it, 4 and 12 bytes behind it, and an odd byte
STARTS = [0, 4, 12, 5]


def _place(ranges, device):
    """One byte buffer full of PATTERN holding every (start offset mod 16, bytes) range between guards -> (buffer, [(offset, bytes)])."""
    spots, at = [], 0
    for start, nbytes in ranges:
        at += GUARD
        at += (start - at) % 16
        spots.append((at, nbytes))
        at += nbytes
    buf = torch.full((at + GUARD + 16,), PATTERN, dtype=torch.uint8, device=device)
    shift = (-buf.data_ptr()) % 16          # offsets are relative to a 16-byte boundary of the address space
    return buf, [(o + shift, n) for o, n in spots]


def run_clear(device, lib, ranges):
    buf, spots = _place(ranges, device)
    for (start, _), (o, _) in zip(ranges, spots):
        assert (buf.data_ptr() + o) % 16 == start
    lib.clear_many([(buf.data_ptr() + o, n) for o, n in spots], buf)
    host = buf.cpu()
    want = torch.full_like(host, PATTERN)
    for o, n in spots:
        want[o: o + n] = 0
    bad = (host != want).nonzero()
    assert bad.numel() == 0, "first wrong byte at %d of %d (ranges %s)" % (int(bad[0]), host.numel(), spots[:4])


def cases():
    every = [(start, n) for n in SIZES for start in STARTS]
    yield "one_member", [(4, 20)]
    yield "one_large_member", [(12, SIZES[5])]
    yield "all_sizes_and_starts", every                      # 40 members
    yield "most_members_of_one_launch", (every + every)[:MAX_MEMBERS]
    yield "more_than_one_launch", (every + every)[:MAX_MEMBERS + 3]
    yield "an_empty_member", [(0, 16), (4, 0), (12, 5)]


CASES = dict(cases())


@pytest.mark.parametrize("name", sorted(CASES))
def test_clear_many_emulated(name):
    run_clear("cpu", emu_lib(), CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_clear_many_gpu(gpu_device, name):
    from lvsr_amd import native
    run_clear(gpu_device, native.get(), CASES[name])
