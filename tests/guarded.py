"""A guarded arena for the workspaces of the device calls (tests/test_gpu_workspace.py): one device allocation that holds
a patterned band, the workspace at a base that is 16-byte aligned and nothing more, and a patterned band behind it.  A
kernel that writes in front of or behind its workspace changes a band, and check() says where."""
import numpy as np

LEAD_PAD = 4096
GUARD = 4096
LEADS = (16, 48, 240)
POISONS = ("zeros", "pattern", "ones")  # the order of the legs: a sizing fault shows on zeros, before any wild index


def torch_mod():
    import torch
    return torch


def pattern(lo, hi):
    """(i * 131 + 7) & 0xFF for the allocation's bytes i in [lo, hi), generated on the device"""
    torch = torch_mod()
    i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
    return ((i * 131 + 7) & 0xFF).to(torch.uint8)


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, nbytes, lead, poison, seed=0):
        torch = torch_mod()
        assert lead in LEADS and nbytes >= 0
        self.nbytes, self.lead = nbytes, lead
        self.front = LEAD_PAD + lead
        self.back = (nbytes + GUARD + 15) // 16 * 16 - nbytes  # GUARD, rounded up so that the whole is a multiple of 16
        self.buf = torch.empty(self.front + nbytes + self.back, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0, "the allocator's base is expected to be 256-byte aligned"
        self.buf[:self.front] = pattern(0, self.front)
        self.buf[self.front + nbytes:] = pattern(self.front + nbytes, self.buf.numel())
        self.ws = self.buf[self.front:self.front + nbytes]
        ptr = self.ws.data_ptr()
        assert ptr == self.buf.data_ptr() + LEAD_PAD + lead and self.ws.numel() == nbytes
        assert ptr % 16 == 0 and ptr % 32 != 0, "the base must be 16-byte aligned and not 32-byte aligned"
        self.fill(poison, seed)

    def fill(self, poison, seed=0):
        """poison: "zeros", "pattern" (seeded random bytes), "ones" (0xFF); "leftover" leaves what is there"""
        torch = torch_mod()
        if poison == "zeros":
            self.ws.zero_()
        elif poison == "ones":
            self.ws.fill_(0xFF)
        elif poison == "pattern":
            rnd = np.random.default_rng(seed).integers(0, 256, self.nbytes, dtype=np.uint8)
            if self.nbytes:
                self.ws.copy_(torch.from_numpy(rnd).cuda())
        else:
            assert poison == "leftover", poison

    def check(self):
        """synchronises; raises GuardError with the first and last changed offset of either band: negative offsets are
        relative to the workspace's start (-1 is the byte in front of it), others to its end (0 is the first byte behind)"""
        torch = torch_mod()
        torch.cuda.synchronize()
        found = []
        end = self.front + self.nbytes
        for name, lo, hi, origin in (("in front of", 0, self.front, self.front), ("behind", end, self.buf.numel(), end)):
            bad = torch.nonzero(self.buf[lo:hi] != pattern(lo, hi)).flatten()
            if bad.numel():
                first, last = int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin
                found.append("%d byte(s) %s the workspace changed, offsets %d .. %d" % (bad.numel(), name, first, last))
                self.changed = (first, last)
        if found:
            raise GuardError("; ".join(found) + " (workspace of %d bytes, lead %d)" % (self.nbytes, self.lead))


def arena(nbytes, lead, poison, seed=0):
    return Arena(nbytes, lead, poison, seed)
