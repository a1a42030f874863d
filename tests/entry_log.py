"""A recorder of the C entries the host code calls: `record(monkeypatch)` puts a proxy in the place of differender_amd._native.lib()
whose every entry notes its name -- and, with with_args=True, its arguments -- and then calls the real function. It launches
nothing itself; what the entries do is untouched."""
import ctypes

from differender_amd import _native as N


def _plain(name, args):
    """The arguments as text: numbers verbatim, pointers as null / ptr (an address differs from run to run)."""
    kinds = N.SIGNATURES[name][1]
    return tuple(("ptr" if a else "null") if k is ctypes.c_void_p else repr(a) for k, a in zip(kinds, args))


class EntryLog:
    def __init__(self, real, with_args=False):
        self.real, self.with_args = real, with_args
        self.names, self.calls = [], []

    def __getattr__(self, name):   # (only what the proxy itself does not have: the library's entries)
        fn = getattr(self.real, name)

        def entry(*args):
            self.names.append(name)
            if self.with_args:
                self.calls.append((name, _plain(name, args)))
            return fn(*args)
        return entry

    def take(self):
        """The names recorded since the last take()."""
        names, self.names = self.names, []
        return names


def record(monkeypatch, with_args=False):
    log = EntryLog(N.lib(), with_args)
    monkeypatch.setattr(N, "lib", lambda: log)
    return log
