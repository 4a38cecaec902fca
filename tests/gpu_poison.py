"""The poisoned device allocator of the GPU tests of the ctypes units (tests/test_{png_encode,png_decode,model_io,scene_images}_gpu.py):
every tensor a run is given lies inside a larger allocation filled with 0xA5, PAD bytes in front of it and PAD bytes behind it, and
guards_intact() asserts that those bytes are still there."""
PAD = 256


class Poisoned:
    def __init__(self):
        self.held = []

    def inside(self, nbytes, offset=0):
        """a uint8 view of nbytes, PAD + offset bytes behind the start of its allocation (offset = 1: an odd address)"""
        import torch
        front = PAD + offset
        whole = torch.full((front + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        view = whole[front:front + nbytes]
        self.held.append((whole, front, view))
        return view

    def alloc(self, nbytes):
        return self.inside(int(nbytes))

    def up(self, t, offset=0):
        """a host tensor -> its copy on the device, inside a poisoned allocation"""
        v = self.inside(t.numel() * t.element_size(), offset).view(t.dtype).reshape(t.shape)
        v.copy_(t)
        return v

    @staticmethod
    def down(t):
        return t.detach().cpu().numpy().copy()

    def clear(self):
        self.held.clear()

    def guards_intact(self):
        """asserts the poison around every tensor handed out -> their number; forgets them"""
        n = 0
        for whole, front, view in self.held:
            assert bool((whole[:front] == 0xA5).all()) and bool((whole[front + view.numel():] == 0xA5).all()), "bytes around a %d-byte tensor were overwritten" % view.numel()
            n += 1
        self.held.clear()
        return n
