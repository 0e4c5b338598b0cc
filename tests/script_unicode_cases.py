"""Group scripts that sweep the script VM's Unicode work (policy-server_amd/csrc/groupvm.hpp: to_upper,
to_lower, make_upper, make_lower, trim) over the whole case tables, shared by the CPU tests
(test_script_unicode.py, test_script_vm.py) and the GPU test (test_script_unicode_gpu.py).

The VM maps non-ASCII code points through a per-script char table that expr.cpp builds at load from
the script's literals, closed under the case mappings; a code point a run can hold but the table
lacks maps to itself and carries no White_Space / Cased / Case_Ignorable bit. Every expected value
here comes straight from CPython's `str.upper()`, `str.lower()` and `str.strip()` (Unicode 13.0.0,
the database the product's table generator reads), never from the product's tables or the oracle.

Every script ends in `&& a()`: it accepts exactly when member `a` accepts and otherwise rejects
with cause `a`. A wrong string result makes the part before `&&` false, so `a` is never called and
the group rejects without a cause, or rejects where it should accept.

Four families (each a list of scripts, deterministic):

* values    every code point >= U+0080 whose upper or lower mapping differs from itself (2,795; 103
            with a multi-character mapping), PER_VALUES to a script, as three arrays: the
            characters, the expected upper strings, the expected lower strings. Per code point five
            comparisons (to_upper, to_lower, the sandwich "a" + c + "b" upper-cased, make_upper and
            make_lower on a copy); each hit adds the code point's position, and the sum is compared
            with a literal.
* closure   the code points whose closure under upper / lower (with U+03C2 wherever U+03A3 appears)
            leaves the characters the script names (113): one script per code point and context
            (alone, "a" + c, c + "b", "a" + c + "b"). The only non-ASCII literal is c. The script
            alternates to_upper / to_lower, from either end, until CPython's results cycle, plus one
            step, and reports through len() and bytes() of every step and the equalities between
            steps. It never names a result: naming one would put it in the table.
* context   Final_Sigma: every assigned code point of the BMP and plane 1 that CPython's rule sees
            as Cased or Case_Ignorable (6,217: 6,160 of them non-ASCII, and the ASCII letters and
            ' . : ^ ` that the VM answers without its table) and a seeded sample of 600 that are neither,
            PER_CONTEXT to a script. Per code point six strings around U+03A3; whether each lowered
            string contains U+03C2 makes a six-bit number that is compared with the expected one;
            each hit adds the code point's position.
* trim      the 25 White_Space code points and nine look-alikes that must stay, at both ends and in
            the middle of a string, alone and beside ASCII blanks; bytes() and len() after trim().

Sums of positive position weights over hits cannot reach the expected literal unless every code
point of the script hits, so two errors in one script cannot cancel."""
import json
import random
import unicodedata

assert unicodedata.unidata_version == "13.0.0"  # the generator's database

PER_VALUES = 40
PER_CONTEXT = 64
SIGMA, FINAL_SIGMA = "Σ", "ς"

# White_Space (PropList.txt, Unicode 13.0), written out by hand (as tests/test_unicode_tables.py)
WHITE_SPACE = sorted(set(range(0x09, 0x0E)) | {0x20, 0x85, 0xA0, 0x1680} | set(range(0x2000, 0x200B)) | {
    0x2028, 0x2029, 0x202F, 0x205F, 0x3000})
# not White_Space: zero-width and format characters, the information separators (str.isspace is
# true for U+001C..U+001F, Rust's char::is_whitespace is not), the Mongolian vowel separator (Zs
# before Unicode 6.3), the soft hyphen
LOOK_ALIKES = [0x200B, 0x200C, 0x200D, 0x2060, 0xFEFF, 0x180E, 0x001C, 0x001F, 0x00AD]


def lit(s):
    """A script string literal: raw UTF-8, escapes only where the language needs them."""
    out = []
    for ch in s:
        if ch in '"\\':
            out.append("\\" + ch)
        elif ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append("\\x%02x" % ord(ch))
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


def _arr(items):
    return "[" + ", ".join(lit(x) if isinstance(x, str) else str(x) for x in items) + "]"


def _scalars():
    return (c for c in range(0x110000) if not 0xD800 <= c < 0xE000)


# ----------------------------------------------------------------------------- values
def value_code_points():
    return [c for c in _scalars() if c >= 0x80 and (chr(c).upper() != chr(c) or chr(c).lower() != chr(c))]


def values_script(cps, bump=0):
    """One script over the code points cps; `bump` is added to the expected sum (a script with
    bump != 0 must reject: the generator is not vacuous)."""
    cs = [chr(c) for c in cps]
    for c in cs:  # upper-casing has no context rule: the sandwich's answer is the parts'
        assert ("a" + c + "b").upper() == "A" + c.upper() + "B"
    n = len(cs)
    want = 5 * n * (n + 1) // 2 + bump
    return (f"let cs = {_arr(cs)}; let us = {_arr([c.upper() for c in cs])}; let ls = {_arr([c.lower() for c in cs])}; "
            f"let n = 0; for j in 0..{n} {{ let c = cs[j]; let w = j + 1; "
            "if c.to_upper() == us[j] { n += w; } if c.to_lower() == ls[j] { n += w; } "
            'if ("a" + c + "b").to_upper() == "A" + us[j] + "B" { n += w; } '
            "let m = c; m.make_upper(); if m == us[j] { n += w; } "
            "let k = c; k.make_lower(); if k == ls[j] { n += w; } } "
            f"n == {want} && a()")


def values_scripts(bump=0):
    cps = value_code_points()
    return [values_script(cps[k:k + PER_VALUES], bump) for k in range(0, len(cps), PER_VALUES)]


# ----------------------------------------------------------------------------- closure
def case_closure(c):
    """The code points reachable from chr(c) by upper / lower, with U+03C2 wherever U+03A3 appears."""
    seen, work = set(), [chr(c)]
    while work:
        x = work.pop()
        if x in seen:
            continue
        seen.add(x)
        work += list(x.upper()) + list(x.lower()) + ([FINAL_SIGMA] if x == SIGMA else [])
    return seen


def closure_code_points():
    out = []
    for c in value_code_points():
        named = {chr(c)} | set(chr(c).upper()) | set(chr(c).lower())
        if any(ord(x) >= 0x80 for x in case_closure(c) - named):
            out.append(c)
    return out


CONTEXTS = (("alone", "", ""), ("after", "a", ""), ("before", "", "b"), ("between", "a", "b"))  # (name, prefix, suffix)


def _chain(s, upper_first):
    """s and its alternating images until (string, next step) repeats, plus one step."""
    steps, seen, up = [s], set(), upper_first
    extra = False
    while True:
        key = (steps[-1], up)
        if key in seen:
            if extra:
                return steps
            extra = True
        seen.add(key)
        steps.append(steps[-1].upper() if up else steps[-1].lower())
        up = not up


def closure_script(c, context, bump=0):
    pre, post = next((p, q) for name, p, q in CONTEXTS if name == context)
    start = pre + chr(c) + post
    expr = " + ".join(lit(x) for x in (pre, chr(c), post) if x)
    parts, checks, names, strings = [f"let s = {expr};"], [], ["s"], [start]
    for tag, upper_first in (("u", True), ("l", False)):
        chain = _chain(start, upper_first)
        prev, up = "s", upper_first
        for k, text in enumerate(chain[1:]):
            name = f"{tag}{k}"
            parts.append(f"let {name} = {prev}.{'to_upper' if up else 'to_lower'}();")
            names.append(name)
            strings.append(text)
            prev, up = name, not up
    for k, (name, text) in enumerate(zip(names, strings)):
        nbytes = len(text.encode()) + (bump if k == len(names) - 1 else 0)
        checks.append(f"{name}.len() == {len(text)} && {name}.bytes() == {nbytes}")
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            checks.append(f"{names[i]} {'==' if strings[i] == strings[j] else '!='} {names[j]}")
    return " ".join(parts) + " " + " && ".join(checks) + " && a()"


def closure_scripts(bump=0):
    return [closure_script(c, ctx, bump) for c in closure_code_points() for ctx, _, _ in CONTEXTS]


# ----------------------------------------------------------------------------- Final_Sigma context
def _assigned():
    return [c for c in range(0x20000) if unicodedata.category(chr(c)) not in ("Cn", "Cs")]


def context_code_points():
    """(the Cased or Case_Ignorable code points, the seeded sample of the others)"""
    seen, rest = [], []
    for c in _assigned():
        hit = FINAL_SIGMA in ("A" + chr(c) + SIGMA).lower() or FINAL_SIGMA in (chr(c) + SIGMA).lower()
        (seen if hit else rest).append(c)
    return seen, sorted(random.Random(0x3C2).sample(rest, 600))


def _sigma_forms(c):
    return ["A" + c + SIGMA, c + SIGMA, "A" + SIGMA + c, "A" + SIGMA + c + "B", "A" + c + SIGMA + c + "B",
            c + SIGMA + c]


def context_script(cps, bump=0):
    cs = [chr(c) for c in cps]
    ws = [sum((FINAL_SIGMA in s.lower()) << b for b, s in enumerate(_sigma_forms(c))) for c in cs]
    n = len(cs)
    S, F = lit(SIGMA), lit(FINAL_SIGMA)
    forms = [f'"A" + c + {S}', f"c + {S}", f'"A{SIGMA}" + c', f'"A{SIGMA}" + c + "B"', f'"A" + c + {S} + c + "B"',
             f"c + {S} + c"]
    body = " ".join(f"if ({f}).to_lower().contains({F}) {{ v += {1 << b}; }}" for b, f in enumerate(forms))
    return (f"let cs = {_arr(cs)}; let ws = {_arr(ws)}; let n = 0; "
            f"for j in 0..{n} {{ let c = cs[j]; let v = 0; {body} if v == ws[j] {{ n += j + 1; }} }} "
            f"n == {n * (n + 1) // 2 + bump} && a()")


def context_scripts(bump=0):
    seen, sample = context_code_points()
    cps = seen + sample
    return [context_script(cps[k:k + PER_CONTEXT], bump) for k in range(0, len(cps), PER_CONTEXT)]


# ----------------------------------------------------------------------------- trim
def trim_script(cps, bump=0):
    ws = "".join(map(chr, WHITE_SPACE))  # Rust's str::trim takes off White_Space, not str.isspace
    cs = [chr(c) for c in cps]
    plain = [(c + "x" + c + "y" + c).strip(ws) for c in cs]
    mixed = [(" " + c + "\t" + "x" + c + " y" + c + "\n").strip(ws) for c in cs]
    n = len(cs)
    return (f"let cs = {_arr(cs)}; let bs = {_arr([len(s.encode()) for s in plain])}; "
            f"let ns = {_arr([len(s) for s in plain])}; let ms = {_arr([len(s.encode()) for s in mixed])}; "
            f"let n = 0; for j in 0..{n} {{ let c = cs[j]; let w = j + 1; "
            'let s = c + "x" + c + "y" + c; s.trim(); if s.bytes() == bs[j] { n += w; } if s.len() == ns[j] { n += w; } '
            'let t = " " + c + "\\t" + "x" + c + " y" + c + "\\n"; t.trim(); if t.bytes() == ms[j] { n += w; } } '
            f"n == {3 * n * (n + 1) // 2 + bump} && a()")


def trim_scripts(bump=0):
    return [trim_script(WHITE_SPACE, bump), trim_script(LOOK_ALIKES, bump),
            trim_script(sorted(WHITE_SPACE + LOOK_ALIKES, key=lambda c: (c * 7919) % 101), bump)]


FAMILIES = {"values": values_scripts, "closure": closure_scripts, "context": context_scripts, "trim": trim_scripts}
_CACHE = {}


def scripts(family, bump=0):
    """The family's scripts (generated once per process)."""
    key = (family, bump)
    if key not in _CACHE:
        _CACHE[key] = FAMILIES[family](bump)
    return _CACHE[key]


# ----------------------------------------------------------------------------- groups and requests
LABELS = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
MEMBER = {"a": {"module": LABELS, "settings": {"mandatory_labels": ["a"]}}}
CHUNK = 64  # groups to an environment: a wave of wide_groups_kernel runs a pass's scripts one after another


def chunks(family, bump=0):
    rows = scripts(family, bump)
    return [rows[k:k + CHUNK] for k in range(0, len(rows), CHUNK)]


def groups_doc(rows):
    return {f"g{k}": {"policies": MEMBER, "expression": e, "message": f"group {k} rejected"}
            for k, e in enumerate(rows)}


def review(accepting, uid):
    """A Pod review that carries label `a` (member a accepts) or no label (member a rejects)."""
    return json.dumps({"apiVersion": "admission.k8s.io/v1", "kind": "AdmissionReview", "request": {
        "uid": uid, "kind": {"group": "", "version": "v1", "kind": "Pod"},
        "resource": {"group": "", "version": "v1", "resource": "pods"}, "operation": "CREATE",
        "namespace": "default", "userInfo": {"username": "u"},
        "object": {"kind": "Pod", "metadata": {"name": "p", "labels": {m: "x" for m in accepting}},
                   "spec": {"containers": [{"name": "c", "image": "nginx"}]}}}})


VECTORS = ["", "a"]
_ORACLES = {}


def oracle_env(family, k, bump=0):
    """The oracle's environment of chunk k of the family: built once, shared by the tests, left unchanged."""
    import oracle as O
    key = (family, k, bump)
    if key not in _ORACLES:
        _ORACLES[key] = O.OracleEnv(groups_doc(chunks(family, bump)[k]), continue_on_errors=True)
    return _ORACLES[key]
