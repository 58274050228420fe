"""flowlogs-pipeline's `transform filter` stage for the device path (include/nfagg.h, "transform filter"): the query language of
pkg/dsl (lexer.go, expr.y) as a parser of its own, and the compiler from a stage's parameters to the atoms, postfix ops and
steps of nfagg_filter_spec.

parse_query(text) returns the tree dsl.Parse builds: ("and" | "or", left, right), ("with" | "without", key) or
("cmp", key, op, value) with op one of = != < > <= >= =~ !~ and value an int or bytes (Go strings are bytes). Errors are
ValueErrors that end in line:column, the position text/scanner holds when the lexer reports (lexer.go:219-221).
OR binds tighter than AND (expr.y:16-17: %left AND, then %left OR; the later line has the higher precedence).

TransformFilter(config, k8s_entries, labels, layer, net_flags) compiles FLP's TransformFilter parameters. Predicates over string
keys (the Kubernetes fields, the subnet labels, K8S_FlowLayer, DnsFlagsResponseCode, IPSecStatus) are evaluated here once per
table row, with `re.search` standing in for RE2 as in metrics.py; the device looks the answer up. What the device does not
serve raises ValueError, and such a stage stays on the host path. Steps, whose index the roll takes: the keep rules in
configuration order, then one step per other rule, a conditional_sampling rule taking one per condition."""
import ctypes as C
import json
import re

from . import _lib as L
from .metrics import K8S_SUFFIXES, _b, _field_present
from .table import K8S_FIELDS, flp_enum_name

# ---------------------------------------------------------------- the lexer (text/scanner's default mode, lexer.go:169-217)
_KEYWORDS = {"and": "AND", "or": "OR", "with": "WITH", "without": "WITHOUT"}
_OPS2 = {"!=": "NEQ", "=~": "REG", "!~": "NREG", ">=": "GE", "<=": "LE"}
_OPS1 = {"=": "EQ", ">": "GT", "<": "LT", "(": "OPEN_PARENTHESIS", ")": "CLOSE_PARENTHESIS"}
_SYMBOL = {"EQ": "=", "NEQ": "!=", "REG": "=~", "NREG": "!~", "GT": ">", "LT": "<", "GE": ">=", "LE": "<="}
_ESC = {"a": 7, "b": 8, "f": 12, "n": 10, "r": 13, "t": 9, "v": 11, "\\": 92, '"': 34}


class _Scanner:
    def __init__(self, text: str):
        self.s, self.i, self.line, self.col = text, 0, 1, 0       # col: the column of the last character read
        self.last_line_len = 0
        self.tok_line, self.tok_col = 1, 0

    def _next(self):
        if self.i >= len(self.s):
            return ""
        ch = self.s[self.i]
        self.i += 1
        if ch == "\n":
            self.line, self.last_line_len, self.col = self.line + 1, self.col, 0
        else:
            self.col += 1
        return ch

    def _peek(self):
        return self.s[self.i] if self.i < len(self.s) else ""

    def error(self, msg):
        raise ValueError("%s: %d:%d" % (msg, self.tok_line, self.tok_col))

    def _mark(self):
        """The position Scan sets: that of the character just read (scanner.go, "set token position")."""
        if self.col > 0:
            self.tok_line, self.tok_col = self.line, self.col
        else:
            self.tok_line, self.tok_col = self.line - 1, self.last_line_len

    def scan(self):
        """(kind, value): kind one of the grammar's tokens, or "" at the end."""
        while True:
            ch = self._next()
            while ch and ch in " \t\n\r":
                ch = self._next()
            self._mark()
            if not ch:
                return "", None
            if ch == "/" and self._peek() in ("/", "*"):          # comments are skipped
                if self._next() == "/":
                    while self._peek() not in ("", "\n"):
                        self._next()
                else:
                    while True:
                        c = self._next()
                        if not c or (c == "*" and self._peek() == "/"):
                            self._next()
                            break
                continue
            break
        start = self.i - 1
        if ch.isalpha() or ch == "_":
            while self._peek().isalnum() or self._peek() == "_":
                self._next()
            text = self.s[start:self.i]
            return _KEYWORDS.get(text.lower(), "NF_FIELD"), text
        if ch.isdigit() or (ch == "." and self._peek().isdigit()):
            # scanNumber: the literal's whole extent, prefixes, separators and exponents included
            based = ch == "0" and self._peek() != "" and self._peek() in "xXbBoO"
            while self._peek().isalnum() or self._peek() in ("_", "."):
                c = self._next()
                if not based and c in "eE" and self._peek() != "" and self._peek() in "+-":
                    self._next()
            lit = self.s[start:self.i]
            is_float = not based and ("." in lit or "e" in lit.lower())
            text = self.s[start:self.i]
            if is_float:
                self.error("Float values are currently unsupported")
            if not text.isdigit() or not text.isascii():
                self.error('strconv.ParseInt: parsing "%s": invalid syntax' % text)
            if int(text) > 2**63 - 1:
                self.error('strconv.ParseInt: parsing "%s": value out of range' % text)
            return "NUMBER", int(text)
        if ch == '"':
            out, closed = bytearray(), False
            while True:
                c = self._next()
                if not c or c == "\n":
                    break
                if c == '"':
                    closed = True
                    break
                if c != "\\":
                    out += c.encode()
                    continue
                e = self._next()
                if e in _ESC:
                    out.append(_ESC[e])
                elif e == "x" or e in "01234567" or e in ("u", "U"):
                    width, base = {"x": (2, 16), "u": (4, 16), "U": (8, 16)}.get(e, (3, 8))
                    digits = e if base == 8 else ""
                    while len(digits) < width:
                        digits += self._next()
                    try:
                        v = int(digits, base)
                    except ValueError:
                        self.error("invalid syntax")
                    if e in ("u", "U"):
                        if v > 0x10FFFF or 0xD800 <= v < 0xE000:
                            self.error("invalid syntax")
                        out += chr(v).encode()
                    elif v > 255:
                        self.error("invalid syntax")
                    else:
                        out.append(v)
                else:
                    closed = False
                    break
            if not closed:
                self.error("invalid syntax")                      # strconv.Unquote of a literal that is not terminated
            return "STRING", bytes(out)
        if ch == "`":
            end = self.s.find("`", self.i)
            if end < 0:
                self.i = len(self.s)
                self.error("invalid syntax")
            raw = self.s[self.i:end]
            for _ in range(end + 1 - self.i):
                self._next()
            return "STRING", raw.replace("\r", "").encode()
        if ch == "'":                                             # a character literal is a token of its own, and a field name
            while self._peek() not in ("", "'", "\n"):
                if self._next() == "\\":
                    self._next()
            self._next()
            return "NF_FIELD", self.s[start:self.i]
        two = ch + self._peek()
        if two in _OPS2:
            self._next()
            return _OPS2[two], two
        return _OPS1.get(ch, "NF_FIELD"), ch


class _Parser:
    def __init__(self, text):
        self.sc = _Scanner(text)
        self.kind, self.value = self.sc.scan()

    def _advance(self):
        kind, value = self.kind, self.value
        self.kind, self.value = self.sc.scan()
        return kind, value

    def _unexpected(self):
        self.sc.error("syntax error: unexpected %s" % (self.kind or "$end"))

    def _expect(self, kind):
        if self.kind != kind:
            self._unexpected()
        return self._advance()[1]

    def expr(self):                                               # AND: the lowest precedence, left-associative
        left = self.or_chain()
        while self.kind == "AND":
            self._advance()
            left = ("and", left, self.or_chain())
        return left

    def or_chain(self):
        left = self.primary()
        while self.kind == "OR":
            self._advance()
            left = ("or", left, self.primary())
        return left

    def primary(self):
        if self.kind == "OPEN_PARENTHESIS":
            self._advance()
            inner = self.expr()
            self._expect("CLOSE_PARENTHESIS")
            return inner
        if self.kind in ("WITH", "WITHOUT"):
            which = self._advance()[0].lower()
            self._expect("OPEN_PARENTHESIS")
            key = self._expect("NF_FIELD")
            self._expect("CLOSE_PARENTHESIS")
            return (which, key)
        key = self._expect("NF_FIELD")
        if self.kind not in _SYMBOL:
            self._unexpected()
        op = self._advance()[0]
        wants = ("STRING", "NUMBER") if op in ("EQ", "NEQ") else ("STRING",) if op in ("REG", "NREG") else ("NUMBER",)
        if self.kind not in wants:
            self._unexpected()
        value = self._advance()[1]
        if op in ("REG", "NREG"):
            try:
                re.compile(value)
            except re.error as e:
                raise ValueError("invalid regex filter: cannot compile regex [%s]" % e)
        return ("cmp", key, _SYMBOL[op], value)


def parse_query(text: str):
    """dsl.Parse's tree of a keep_entry_query (see the module's docstring)."""
    p = _Parser(text)
    tree = p.expr()
    if p.kind:
        p._unexpected()
    return tree


# ---------------------------------------------------------------- keys
NUM_FIELDS = {"Etype": 0, "Bytes": 1, "Packets": 2, "Sampling": 3, "Proto": 4, "Dscp": 5, "SrcPort": 6, "DstPort": 7, "IcmpType": 8, "IcmpCode": 9,
              "Flags": 10, "TimeFlowStartMs": 11, "TimeFlowEndMs": 12, "FlowDirection": 13, "TimeFlowRttNs": 14, "DnsLatencyMs": 15, "DnsId": 16,
              "DnsFlags": 17, "DnsErrno": 18, "PktDropBytes": 19, "PktDropPackets": 20, "PktDropLatestFlags": 21, "IPSecRetCode": 22}
PRESENCE_FIELDS = {"SrcAddr": 23, "DstAddr": 24, "SrcMac": 25, "DstMac": 26}
ALWAYS_OTHER = {"Interfaces": "list", "IfDirections": "list", "AgentIP": "string", "TimeReceived": "number"}      # decode_protobuf.go:63-82
REFUSED = ("_HashId", "_RecordType", "Udns", "DnsName", "TLSVersion", "TLSTypes", "TLSCipherSuite", "TLSGroup", "QuicVersion", "QuicSeenLongHdr",
           "QuicSeenShortHdr")
ATOM_CONST, ATOM_NUM, ATOM_PRESENT, ATOM_TABLE, ATOM_ADDR, ATOM_MAC = range(6)
CMP = {"=": 0, "!=": 1, "<": 2, ">": 3, "<=": 4, ">=": 5}
DIM_SRC_K8S_ROW, DIM_DST_K8S_ROW, DIM_SRC_SUBNET_LABEL, DIM_DST_SUBNET_LABEL, DIM_FLOW_LAYER, DIM_DNS_RCODE, DIM_IPSEC_STATUS = range(7)
OP_AND, OP_OR, OP_NOT = 0x80, 0x81, 0x82
STEP_KEEP, STEP_REMOVE, STEP_SAMPLE_IF = range(3)
MAX_ATOMS, MAX_OPS, MAX_STEPS, MAX_STACK, NO_RULE = 64, 256, 32, 32, 0xFF
STORE_SAMPLING = 1
_MUTATING = ("remove_field", "add_field", "add_field_if_doesnt_exist", "add_field_if", "add_regex_if", "add_label", "add_label_if")
_INT = re.compile(rb"[+-]?[0-9]+\Z")


def go_ip_string(ip16: bytes) -> bytes:
    """net.IP.String() of a 16-byte address: dotted for a v4-mapped one, else lower-case hextets with the longest run of two or
    more zero hextets (the first of equals) as ::."""
    ip16 = bytes(ip16)
    if ip16[:12] == bytes(10) + b"\xff\xff":
        return b"%d.%d.%d.%d" % tuple(ip16[12:])
    h = [int.from_bytes(ip16[k:k + 2], "big") for k in range(0, 16, 2)]
    best, best_len, k = -1, 1, 0
    while k < 8:
        j = k
        while j < 8 and h[j] == 0:
            j += 1
        if j - k > best_len:
            best, best_len = k, j - k
        k = j + 1 if j == k else j
    if best < 0:
        return b":".join(b"%x" % x for x in h)
    return b":".join(b"%x" % x for x in h[:best]) + b"::" + b":".join(b"%x" % x for x in h[best + best_len:])


def _parse_int(s: bytes):
    """ConvertToInt of a string: strconv.ParseInt(s, 10, 64), None where it fails (convert.go:196-198)."""
    if not _INT.match(s):
        return None
    v = int(s)
    return v if -2**63 <= v < 2**63 else None


def _compare(v: int, op: str, n: int) -> bool:
    return {"=": v == n, "!=": v != n, "<": v < n, ">": v > n, "<=": v <= n, ">=": v >= n}[op]


def filter_roll(seed: int, flow_index: int, step: int, value: int) -> bool:
    """nfagg_filter_roll, restated: the device path's roll of step `step` for the flow with running index flow_index."""
    if value == 0:
        return True
    m, k = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def fmix(x):
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & m
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & m
        return x ^ (x >> 33)
    return fmix(fmix((seed + k * flow_index) & m) ^ (k * (step + 1) & m)) % value == 0


class TransformFilter:
    """FLP's TransformFilter parameters (a dict or JSON text: rules, samplingField) compiled for nfagg_filter_create.
    k8s_entries: the Kubernetes table's [(ip, info)] (None: no table); labels: the net table's label texts (None: no table);
    layer: the Kubernetes table has a layer; net_flags: the net table's flags (L.NET_DECODE_TCP_FLAGS decides what Flags is).
    atoms: [dict(kind=..., ...)], ops: bytes, steps: [(kind, group, value, op_begin, op_count)], flags. ValueError for a stage the
    device does not serve: field-mutating rules, $(..) variables, castInt, a rule's number against a key that holds a Go int
    (FlowDirection; Sampling under samplingField, once a keep rule has stored it), a regex or a string equality on a key that is neither
    an address, a MAC nor table-backed, a samplingField other than Sampling, _HashId / _RecordType, Udns, DnsName and the TLS and
    QUIC texts, a key nobody writes, more atoms, ops, steps or stack than the device's limits."""

    def __init__(self, config, k8s_entries=None, labels=None, layer=False, net_flags=0):
        cfg = json.loads(config) if isinstance(config, (str, bytes)) else dict(config or {})
        self.k8s_entries = list(k8s_entries) if k8s_entries is not None else None
        self.labels = [_b(x) for x in labels] if labels is not None else None
        self.layer, self.net_flags = bool(layer), net_flags
        self.atoms, self.ops, self.steps = [], bytearray(), []
        field = cfg.get("samplingField") or ""
        if field not in ("", "Sampling"):
            raise ValueError("samplingField %r: only Sampling is served" % field)
        self.flags = STORE_SAMPLING if field else 0
        keeps, others = [], []
        for rule in cfg.get("rules") or []:
            (keeps if rule.get("type") == "keep_entry_query" else others).append(rule)       # configure, transform_filter.go:241-254
        for rule in keeps:
            self._step(STEP_KEEP, 0, int(rule.get("keepEntrySampling") or 0), lambda r=rule: self._tree(parse_query(r.get("keepEntryQuery") or "")))
        group = 0
        for rule in others:
            t = rule.get("type")
            if t in _MUTATING:
                raise ValueError("rule %r changes fields: the stage stays on the host path" % t)
            if t in ("remove_entry_if_exists", "remove_entry_if_doesnt_exist", "remove_entry_if_equal", "remove_entry_if_not_equal"):
                self._step(STEP_REMOVE, 0, 0, lambda r=rule, t=t: self._remove_entry(t, r.get("removeEntry") or {}))
            elif t == "remove_entry_all_satisfied":
                self._step(STEP_REMOVE, 0, 0, lambda r=rule: self._all(r.get("removeEntryAllSatisfied") or []))
            elif t == "conditional_sampling":
                if group > 31:
                    raise ValueError("more than 32 conditional_sampling rules")
                for cond in rule.get("conditionalSampling") or []:
                    self._step(STEP_SAMPLE_IF, group, int(cond.get("value") or 0), lambda c=cond: self._all(c.get("rules") or []))
                group += 1
            else:
                raise ValueError("unknown rule type %r" % t)

    # -- emitting
    def _step(self, kind, group, value, emit):
        if not 0 <= value <= 0xFFFF:
            raise ValueError("a sampling value of %d is no uint16" % value)
        begin = len(self.ops)
        depth = emit()
        assert depth == 1
        if len(self.ops) > MAX_OPS or len(self.steps) >= MAX_STEPS:
            raise ValueError("the filter has more than %d ops or %d steps" % (MAX_OPS, MAX_STEPS))
        self.steps.append((kind, group, value, begin, len(self.ops) - begin))

    def _atom(self, **a):
        if a not in self.atoms:
            if len(self.atoms) >= MAX_ATOMS:
                raise ValueError("the filter has more than %d atoms" % MAX_ATOMS)
            self.atoms.append(a)
        self.ops.append(self.atoms.index(a))
        return 1

    def _const(self, v):
        return self._atom(kind=ATOM_CONST, value_const=1 if v else 0)

    def _not(self, depth):
        self.ops.append(OP_NOT)
        return depth

    def _tree(self, t, depth=0):
        """Postfix of a parsed tree; returns the stack it leaves (1). depth: the stack below it, for the limit."""
        if t[0] in ("and", "or"):
            self._tree(t[1], depth)
            self._tree(t[2], depth + 1)
            if depth + 2 > MAX_STACK:
                raise ValueError("the query needs a stack deeper than %d" % MAX_STACK)
            self.ops.append(OP_AND if t[0] == "and" else OP_OR)
            return 1
        if t[0] == "with":
            return self._present(t[1])
        if t[0] == "without":
            return self._not(self._present(t[1]))
        _, key, op, value = t
        if op == "!~" or (op == "!=" and not isinstance(value, int)):
            return self._not(self._cmp(key, "=" if op == "!=" else "=~", value))      # NotEqual, NotRegex: negations, true for an absent key
        return self._cmp(key, op, value)

    # -- rules
    def _remove_entry(self, t, g):
        key, value = g.get("input") or "", g.get("value")
        if g.get("castInt"):
            raise ValueError("castInt is not served")
        if t == "remove_entry_if_exists":
            return self._present(key)
        if t == "remove_entry_if_doesnt_exist":
            return self._not(self._present(key))
        if not isinstance(value, (str, bytes)):
            # interface{} == between a YAML number, bool or null and a uint8..uint64 / int64 / string value: never equal
            # (transform_filter.go:111-122), so if_equal never removes and if_not_equal removes whenever the key exists
            # two keys hold a Go int, which a decoder that yields int (not float64) does equal: FlowDirection, and Sampling once
            # storeSampling has written it (transform_filter.go:227)
            if isinstance(value, int) and not isinstance(value, bool) and (key == "FlowDirection" or (key == "Sampling" and self.flags & STORE_SAMPLING)):
                raise ValueError("a number against %s: the reference's answer depends on the YAML decoder's type" % key)
            return self._const(False) if t == "remove_entry_if_equal" else self._present(key)
        if t == "remove_entry_if_equal":
            return self._cmp(key, "=", _b(value))
        self._present(key)
        self._not(self._cmp(key, "=", _b(value)))
        self.ops.append(OP_AND)
        return 1

    def _all(self, rules):
        if not rules:
            return self._const(True)                              # isRemoveEntrySatisfied over no rule (181-189)
        for k, r in enumerate(rules):
            t = r.get("type")
            if t not in ("remove_entry_if_exists", "remove_entry_if_doesnt_exist", "remove_entry_if_equal", "remove_entry_if_not_equal"):
                raise ValueError("rule type %r inside a rule list" % t)
            self._remove_entry(t, r.get("removeEntry") or {})
            if k:
                self.ops.append(OP_AND)
        return 1

    # -- predicates
    def _check_key(self, key):
        if key in REFUSED:
            raise ValueError("key %r is not served on the device" % key)

    def _rows(self, key):
        """(dim, [value bytes or None per truth entry]) of a table-backed string key, or None."""
        for side, prefix, dim in ((0, "SrcK8S_", DIM_SRC_K8S_ROW), (1, "DstK8S_", DIM_DST_K8S_ROW)):
            if key.startswith(prefix) and key[len(prefix):] in K8S_SUFFIXES:
                if self.k8s_entries is None:
                    raise ValueError("key %r needs the Kubernetes table" % key)
                f = K8S_SUFFIXES.index(key[len(prefix):])
                return dim, [_b(info.get(K8S_FIELDS[f]) or b"") if _field_present(info, f) else None for _, info in self.k8s_entries] + [None]
        if key in ("SrcSubnetLabel", "DstSubnetLabel"):
            if self.labels is None:
                raise ValueError("key %r needs the net table" % key)
            return (DIM_SRC_SUBNET_LABEL if key[0] == "S" else DIM_DST_SUBNET_LABEL), [x if x else None for x in self.labels] + [None]
        if key == "K8S_FlowLayer":
            if self.k8s_entries is None:
                raise ValueError("key %r needs the Kubernetes table" % key)
            return DIM_FLOW_LAYER, [b"infra", b"app", None] if self.layer else [None, None, None]
        if key == "DnsFlagsResponseCode":
            return DIM_DNS_RCODE, [flp_enum_name(L.FLP_ENUM_DNS_RCODE, k) for k in range(16)] + [None]
        if key == "IPSecStatus":
            return DIM_IPSEC_STATUS, [b"success", b"error", None]
        return None

    def _table(self, dim, truth):
        return self._atom(kind=ATOM_TABLE, dim=dim, truth=bytes(1 if x else 0 for x in truth))

    def _present(self, key):
        self._check_key(key)
        if key in NUM_FIELDS or key in PRESENCE_FIELDS:
            if key in ("SrcMac", "DstMac"):
                return self._const(True)
            return self._atom(kind=ATOM_PRESENT, field=NUM_FIELDS.get(key, PRESENCE_FIELDS.get(key)))
        if key in ALWAYS_OTHER:
            return self._const(True)
        rows = self._rows(key)
        if rows is None:
            raise ValueError("key %r is not served on the device" % key)
        return self._table(rows[0], [v is not None for v in rows[1]])

    def _cmp(self, key, op, value):
        """One of = < > <= >= =~, and != with a number: NumNotEquals is a comparison of its own, false for an absent key
        (filters.go:74-76, 94-103). The negated string forms are the caller's NOT."""
        self._check_key(key)
        if op == "=" and isinstance(value, bytes) and re.search(rb"\$\([^\)]+\)", value):
            raise ValueError("a $(Key) variable in %r is not served" % value)
        numeric = isinstance(value, int)
        rows = self._rows(key)
        if rows is not None:
            dim, values = rows
            if numeric:
                ints = [_parse_int(v) if v is not None else None for v in values]
                return self._table(dim, [x is not None and _compare(x, op, value) for x in ints])
            if op == "=~":
                rx = re.compile(value)
                return self._table(dim, [v is not None and rx.search(v) is not None for v in values])
            return self._table(dim, [v is not None and v == value for v in values])
        if key in NUM_FIELDS:
            if numeric:
                return self._atom(kind=ATOM_NUM, field=NUM_FIELDS[key], cmp=CMP[op], value=value)
            if op == "=":
                return self._const(False)                         # a string never equals a number (filters.go:57-62)
            raise ValueError("a regex on the numeric key %r is not served" % key)
        if key in PRESENCE_FIELDS:
            if numeric:
                return self._const(False)                         # ParseInt of an address or a MAC fails (convert.go:196-198)
            if op == "=~":
                raise ValueError("a regex on %r is not served" % key)
            side = 1 if key.startswith("Dst") else 0
            if key.endswith("Mac"):
                m = re.match(rb"([0-9a-f]{2}(?::[0-9a-f]{2}){5})\Z", value)          # net.HardwareAddr.String()
                return self._atom(kind=ATOM_MAC, side=side, bytes=bytes.fromhex(value.replace(b":", b"").decode())) if m else self._const(False)
            try:
                import ipaddress
                ip = ipaddress.ip_address(value.decode())
                b16 = ip.packed if len(ip.packed) == 16 else bytes(10) + b"\xff\xff" + ip.packed
            except ValueError:
                return self._const(False)
            return self._atom(kind=ATOM_ADDR, side=side, bytes=b16) if go_ip_string(b16) == value else self._const(False)
        if key in ALWAYS_OTHER:
            if op == "=" and not numeric and ALWAYS_OTHER[key] != "string":
                return self._const(False)
            if numeric and ALWAYS_OTHER[key] == "list":
                return self._const(False)                         # a slice fails ConvertToInt
            raise ValueError("a comparison on %r is not served" % key)
        raise ValueError("key %r is not served on the device" % key)

    # -- the C structures
    def spec(self):
        """(nfagg_filter_spec, the objects it points into: keep them alive for the call)."""
        atoms = (L.FilterAtom * max(len(self.atoms), 1))()
        keep = [atoms]
        for k, a in enumerate(self.atoms):
            atoms[k].kind = a["kind"]
            atoms[k].field, atoms[k].cmp, atoms[k].dim, atoms[k].side = a.get("field", 0), a.get("cmp", 0), a.get("dim", 0), a.get("side", 0)
            atoms[k].value_const, atoms[k].value = a.get("value_const", 0), a.get("value", 0)
            if "bytes" in a:
                atoms[k].bytes[:len(a["bytes"])] = list(a["bytes"])
            if "truth" in a:
                buf = (C.c_uint8 * len(a["truth"])).from_buffer_copy(a["truth"])
                keep.append(buf)
                atoms[k].truth, atoms[k].n_truth = C.cast(buf, C.c_void_p), len(a["truth"])
        ops = (C.c_uint8 * max(len(self.ops), 1)).from_buffer_copy(bytes(self.ops) or b"\0")
        steps = (L.FilterStep * max(len(self.steps), 1))(*[L.FilterStep(*s) for s in self.steps])
        keep += [ops, steps]
        s = L.FilterSpec(C.sizeof(L.FilterSpec), self.flags, len(self.atoms), len(self.ops), len(self.steps), 0, C.cast(atoms, C.c_void_p),
                         C.cast(ops, C.c_void_p), C.cast(steps, C.c_void_p))
        return s, keep


class StageFilter:
    """A compiled filter as a pipeline stage: the Filter of FlowTable.filter(), the roll's seed and the running first_index, so
    that consecutive evictions do not reuse rolls. The stage sits behind the two resolves and in front of every encoder and
    fold: apply() resolves the rows the program reads, runs nfagg_filter_apply and gathers the side arrays of the kept flows."""

    def __init__(self, flt, seed: int = 0):
        self.flt, self.seed, self.first_index = flt, seed, 0
        self.seen = self.kept = self.deferred = 0

    def apply(self, table, recs, k8s=None, net=None, agent_ip=None, now_ns: int = 0, mono_ns: int = 0, present=None, parts=None, rows=None):
        """Returns (kept records with their sampling rewritten, present, parts, network-event rows, held). held lists the flows
        the host must format itself because their stored Sampling does not fit the record's 32 bits, as (position among the
        kept, the admitting keep step, the Sampling the reference stores: max(sampling, 1) * that step's keepEntrySampling)."""
        k8s_rows = table.k8s_resolve(k8s, recs) if k8s is not None else None
        net_rows = table.net_resolve(net, recs, k8s, k8s_rows, agent_ip) if net is not None else None
        _, keep, rule, idx, out, n_kept, n_def = table.filter_apply(self.flt, recs, k8s_rows, net_rows, (present, parts) if present is not None else None, now_ns,
                                                                 mono_ns & ((1 << 64) - 1), self.seed, self.first_index)
        self.first_index += len(keep)
        self.seen, self.kept, self.deferred = self.seen + len(keep), self.kept + n_kept, self.deferred + n_def
        if present is not None:
            present = table.gather(present, idx)
            # the raw network-events part stays behind: once resolved, the encoders read the flows' rows
            parts = {k: (table.gather(v, idx) if v is not None else None) for k, v in (parts or {}).items() if k != "network_events"}
        if rows is not None:
            rows = table.gather(rows, idx)
        held = []
        if n_def:
            steps = self.flt.steps
            for j, i in enumerate(idx.tolist()):
                if keep[i] == 2:
                    r = int(rule[i])
                    held.append((j, r, max(int(out["metrics"]["sampling"][j]), 1) * steps[r][2]))
        return out, present, parts, rows, held
