"""A one-command-at-a-time model of the byte-level string commands (GETRANGE / SETRANGE / APPEND / GET / SET /
STRLEN, RBinaryStream's truncate script) over `bytearray` values, for rbx_string_* and rbx_string_stream.

The rules are [redis-7.2] t_string.c's, transcribed command by command (DESIGN 11.12 marks them as external: nobody
here can run redis).  A key holds a string -- the EMPTY string is a value of its own, not a missing key --, may have
a timeout, or holds another type (an HLL, a {name}:config hash), which every command here but SET refuses with
WRONGTYPE.  A command that fails changes nothing."""
import copy

KMAX = 1 << 29  # proto-max-bulk-len, and the engine's 2^32-bit cap
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

GETRANGE, SETRANGE, APPEND, GET = 0, 1, 2, 3  # RBX_STR_*
OFFSET, WRONGTYPE, TOO_BIG, ILLEGAL = "offset out of range", "WRONGTYPE", "string exceeds maximum", "illegal argument"
OK, NIL, FAILED = 0, 1, 0xFF  # a stream command's status


class Failed(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def getrange_of(s, start, end):
    """getrangeCommand on the string s"""
    strlen = len(s)
    if start < 0 and end < 0 and start > end:
        return b""
    if start < 0:
        start = strlen + start
    if end < 0:
        end = strlen + end
    if start < 0:
        start = 0
    if end < 0:
        end = 0
    if end >= strlen:
        end = strlen - 1
    if start > end or strlen == 0:
        return b""
    return bytes(s[start:end + 1])


class Strings:
    def __init__(self):
        self.data = {}        # name -> bytearray, possibly empty
        self.timeout = set()  # names with a timeout
        self.other = set()    # names that hold another type (HLL, config hash)

    def _string(self, key):
        """the value, None for a missing key"""
        if key in self.other:
            raise Failed(WRONGTYPE)
        return self.data.get(key)

    def exists(self, key):
        return key in self.data or key in self.other

    def ttl(self, key):
        return "missing" if not self.exists(key) else "set" if key in self.timeout else "none"

    def strlen(self, key):
        s = self._string(key)
        return 0 if s is None else len(s)

    def get(self, key):
        s = self._string(key)
        return None if s is None else bytes(s)

    def mget(self, keys):
        """MGET: a key of another type is nil, nothing is raised"""
        return [bytes(self.data[k]) if k in self.data and k not in self.other else None for k in keys]

    def set(self, key, value):
        """SET: replaces whatever the key held, type included, and drops the timeout"""
        self.other.discard(key)
        self.timeout.discard(key)
        self.data[key] = bytearray(value)

    def getrange(self, key, start, end):
        s = self._string(key)
        return getrange_of(s if s is not None else b"", start, end)

    def setrange(self, key, offset, value):
        if offset < 0:  # before the key is looked at
            raise Failed(OFFSET)
        s = self._string(key)
        if len(value) == 0:  # the current length; nothing is created, and there is no size check
            return 0 if s is None else len(s)
        if offset + len(value) > KMAX:
            raise Failed(TOO_BIG)
        if s is None:
            s = self.data[key] = bytearray()
        if len(s) < offset + len(value):
            s.extend(bytes(offset + len(value) - len(s)))  # sdsgrowzero
        s[offset:offset + len(value)] = value
        return len(s)

    def append(self, key, value):
        s = self._string(key)
        if s is None:  # created holding the value, the empty one too
            if len(value) > KMAX:  # (such an argument cannot arrive)
                raise Failed(TOO_BIG)
            self.data[key] = bytearray(value)
            return len(value)
        if len(s) + len(value) > KMAX:
            raise Failed(TOO_BIG)
        s.extend(value)
        return len(s)

    def truncate(self, key, size):
        """RedissonBinaryStream.java:181-190, line by line"""
        length = self.strlen(key)                               # local len = redis.call('strlen', KEYS[1]);
        if size >= length:                                      # if tonumber(ARGV[1]) >= len then
            return                                              #     return; end;
        limited = self.getrange(key, 0, size - 1)               # redis.call('getrange', KEYS[1], 0, tonumber(ARGV[1])-1);
        self.set(key, limited)                                  # redis.call('set', KEYS[1], limitedValue);

    # ---- one command of a stream, and the stream as n single calls ----
    def command(self, key, op, a, b, value):
        """-> (reply bytes or None, reply number, status); raises Failed"""
        if op == GETRANGE:
            r = self.getrange(key, a, b)
            return r, len(r), OK
        if op == GET:
            r = self.get(key)
            return (b"", 0, NIL) if r is None else (r, len(r), OK)
        n = self.setrange(key, a, value) if op == SETRANGE else self.append(key, value)
        return None, n, OK

    def stream(self, names, cmd_key, cmds, vals, cap):
        """cmds: (op, a, b, val_off, val_len) per command.  -> dict(kind, replies, status, off, out, total): kind is
        None, ILLEGAL (nothing ran; off / total are exact when the only error is total > cap) or the first failing
        command's kind."""
        for k, (op, _a, _b, vo, vl) in zip(cmd_key, cmds):
            if k >= len(names) or op > GET or (op in (SETRANGE, APPEND) and (vo > len(vals) or vl > len(vals) - vo)):
                return dict(kind=ILLEGAL, replies=None, status=None, off=None, out=None, total=None)
        trial = copy.deepcopy(self)
        replies, status, off, out, first = [], [], [0], bytearray(), None
        for k, (op, a, b, vo, vl) in zip(cmd_key, cmds):
            try:
                data, num, st = trial.command(names[k], op, a, b, vals[vo:vo + vl] if op in (SETRANGE, APPEND) else b"")
            except Failed as e:
                data, num, st = None, 0, FAILED
                first = first or e.kind
            replies.append(num)
            status.append(st)
            out += data or b""
            off.append(len(out))
        if len(out) > cap:  # refused before any write
            return dict(kind=ILLEGAL, replies=None, status=None, off=off, out=None, total=len(out))
        self.data, self.timeout, self.other = trial.data, trial.timeout, trial.other
        return dict(kind=first, replies=replies, status=status, off=off, out=bytes(out), total=len(out))
