"""Stand-ins for a HipDevice in the CPU tests: MerkleTree and MerkleForest built over them have no GPU behind them, so a
host-side check that comes too late shows as a touched device."""


class NoDevice:
    """Any attribute access is a device call: the host-side checks must raise before one."""

    def __getattr__(self, name):
        raise AssertionError(f"device touched: {name}")


class NoDeviceAt:
    """Stands where a HipDevice would, with its index and its scope(): any device call is an AttributeError."""

    def __init__(self, index):
        self.index = index

    def scope(self):
        from vk_merkle_roots_amd import engine
        return engine.BufferScope(self)
