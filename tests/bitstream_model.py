"""A model of rbx_bitset_stream: a dict of bytearrays to which the commands are applied one at a time, in
array order ([redis-7.2] SETBIT / GETBIT as DESIGN section 11 restates them, and the pipelined-batch rule:
a failing command fails alone).  Shares no code with the engine."""

GETBIT, SETBIT0, SETBIT1 = 0, 1, 2
FAILED = 0xFF
OFFSET_LIMIT = 1 << 32
OK, E_ILLEGAL_ARGUMENT, E_WRONGTYPE, E_REDIS = 0, -1, -5, -9


class StreamModel:
    """strings: name -> bytearray of the keys that exist; wrong: the names that hold another type."""

    def __init__(self, strings=None, wrong=()):
        self.strings = {bytes(k): bytearray(v) for k, v in (strings or {}).items()}
        self.wrong = {bytes(k) for k in wrong}

    def getbit(self, name: bytes, index: int) -> int:
        s = self.strings.get(name)
        byte = index >> 3
        if s is None or byte >= len(s):
            return 0
        return (s[byte] >> (7 - (index & 7))) & 1

    def setbit(self, name: bytes, index: int, value: int) -> int:
        s = self.strings.setdefault(name, bytearray())
        byte = index >> 3
        if byte >= len(s):
            s.extend(bytes(byte + 1 - len(s)))
        mask = 0x80 >> (index & 7)
        old = 1 if s[byte] & mask else 0
        s[byte] = (s[byte] | mask) if value else (s[byte] & ~mask & 0xFF)
        return old

    def run(self, names, cmd_key, cmd_op, cmd_index):
        """(return code, replies): the caller's errors first, with nothing changed; then each command."""
        names = [bytes(n) for n in names]
        if any(k >= len(names) or op > 2 for k, op in zip(cmd_key, cmd_op)):
            return E_ILLEGAL_ARGUMENT, None
        rc, replies = OK, []
        for k, op, index in zip(cmd_key, cmd_op, cmd_index):
            name = names[k]
            code = E_REDIS if index >= OFFSET_LIMIT else (E_WRONGTYPE if name in self.wrong else OK)
            if code != OK:
                rc = rc or code
                replies.append(FAILED)
            elif op == GETBIT:
                replies.append(self.getbit(name, index))
            else:
                replies.append(self.setbit(name, index, op - 1))
        return rc, replies
