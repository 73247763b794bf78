"""Scratch buffers that the launches keep between calls: one uint8 tensor per key, the key composed by the caller (device, stream, and whatever else the
buffer's layout depends on -- two streams never share a buffer).  No GPU is needed to use the class: the device is an argument of get()."""
import torch


class ScratchCache:
    """key -> uint8 tensor.
    zeroed: a new buffer is filled with zeros (the kernels that keep sync words in it re-arm them themselves after that).
    max_entries: a request that has to allocate while the cache holds more than this drops the whole cache first (None: no cap).
    on_drop: called with every buffer before the cache lets go of it (replaced by a larger one, drop(), clear(), the cap)."""

    def __init__(self, zeroed=False, max_entries=None, on_drop=None):
        self.zeroed, self.max_entries, self.on_drop = zeroed, max_entries, on_drop
        self._bufs = {}

    def get(self, key, nbytes, device):
        """the buffer of `key`, at least nbytes long: the cached one where it is large enough, else a new one of nbytes -- the old one is released BEFORE
        the new one is allocated (never both alive).  nbytes == 0 with nothing cached: None."""
        cur = self._bufs.get(key)
        if cur is not None and cur.numel() >= nbytes:
            return cur
        if nbytes == 0:
            return None
        del cur
        self.drop(key)
        if self.max_entries is not None and len(self._bufs) > self.max_entries:
            self.clear()
        buf = self._bufs[key] = (torch.zeros if self.zeroed else torch.empty)(nbytes, dtype=torch.uint8, device=device)
        return buf

    def drop(self, key):
        """let go of the buffer of `key` (absent: nothing happens)"""
        buf = self._bufs.pop(key, None)
        if buf is not None and self.on_drop is not None:
            self.on_drop(buf)

    def clear(self):
        for key in list(self._bufs):
            self.drop(key)

    def values(self):
        return list(self._bufs.values())
