"""Hand-written expectations for policy-group expressions beyond the bool-only subset (VERDICT r04
"What's missing" 1). Each row states what rhai 1.21.0 answers (upstream policy-evaluator v0.24.0,
Cargo.lock:5116-5118, run by evaluation_environment.rs:587-651), written from the language's
documented semantics, not from either implementation here: it is the independent pin the product
(expr.cpp, groupvm.hpp) and the oracle (oracle/rhaisub.py) are both checked against. rhai itself cannot
run in this image, so rows that no reference-held vector covers are parity unpinned.

Members a, b, c are safe-labels policies with one mandatory label each ("a", "b", "c"): a request
carrying the label accepts that member, one without it rejects it. A row is
  (expression, cases) with cases = [(accepting members, expected)], expected one of
    True / False              the group's bool (False: rejected with the causes below)
    ("causes", {..})          rejected; exactly these members are the causes
    ("error", "text")         a 500 whose message contains text (an evaluation error on that path)
Rows in INVALID fail at load (validate_settings runs the script with every member true): the
init error must contain the text."""

VALID = [
    # VERDICT r04 probes
    ("[a(), b()].contains(false)", [("ab", ("causes", set())), ("a", True), ("", True)]),
    ("a() in [true]", [("a", True), ("", ("causes", {"a"}))]),
    ("switch a() { true => b(), _ => false }",
     [("ab", True), ("a", ("causes", {"b"})), ("b", ("causes", {"a"}))]),
    ("a() ?? b()", [("a", True), ("b", ("causes", {"a"}))]),
    ('a().to_string() == "true"', [("a", True), ("", ("causes", {"a"}))]),
    ("let n = 0; if b() { n += 1; } n > 0", [("b", True), ("a", ("causes", {"b"}))]),
    # arrays
    ("let xs = [a(), b(), c()]; xs.len() == 3 && xs[0]", [("a", True), ("bc", ("causes", {"a"}))]),
    ("let cnt = 0; for ok in [a(), b(), c()] { if ok { cnt += 1; } } cnt >= 2",
     [("ac", True), ("abc", True), ("c", ("causes", {"a", "b"})), ("", ("causes", {"a", "b", "c"}))]),
    ("let a1 = [1, 2]; a1.push(3); a1 == [1, 2, 3] && a()", [("a", True)]),
    ("let a1 = [1, 2]; a1 += 3; a1 += [4, 5]; a1.len() == 5 && a1[4] == 5 && a()", [("a", True)]),
    ("let a1 = [1, 2, 3]; a1[-1] == 3 && a1[-3] == 1 && a1[0] == 1 && a()", [("a", True)]),
    ("let a1 = [1]; a1[0] = 5; a1[0] += 1; a1[-1] == 6 && a()", [("a", True)]),
    ("let a1 = [[1, 2], [3]]; a1[1] == [3] && [[1, 2], [3]].contains([1, 2]) && a()", [("a", True)]),
    ("[] == [] && [1] != [1, 2] && [1] != [\"1\"] && [()] == [()] && a()", [("a", True)]),
    ("[1, 2] + [3] == [1, 2, 3] && [].is_empty() && ![0].is_empty() && a()", [("a", True)]),
    # r06: push's receiver is rhai's `&mut` parameter and its result is (); function-call style
    # works on a copy (r05's table wrongly had push([1], 2) == [1, 2])
    ("push([1], 2) == () && a()", [("a", True)]),
    ("let v = [1]; push(v, 2); v == [1] && a()", [("a", True)]),  # function-call style: a copy
    ("a() in [true, b()]", [("a", True), ("ab", True), ("", True), ("b", ("causes", {"a"}))]),
    ('"b" !in ["a"] && a()', [("a", True)]),
    # ranges
    ("2 in 1..3 && !(3 in 1..3) && 3 in 1..=3 && -1 !in 0..5 && a()", [("a", True)]),
    ("let s = 0; for i in 1..=4 { s += i; } s == 10 && a()", [("a", True)]),
    ("let s = 0; for i in range(0, 4) { s += i; } s == 6 && a()", [("a", True)]),
    ("let s = 0; for i in 5..2 { s += 1; } s == 0 && a()", [("a", True)]),
    ('let s = ""; for (x, i) in ["p", "q"] { s += x + i; } s == "p0q1" && a()', [("a", True)]),
    ("let k = 0; for (x, i) in 10..13 { k += x * i; } k == 0 + 11 + 24 && a()", [("a", True)]),
    # switch
    ("switch 3 { 1 | 2 => false, 3..5 => a(), _ => b() }", [("a", True), ("b", ("causes", {"a"}))]),
    ("switch 7 { 1 | 2 => false, 3..5 => a(), _ => b() }", [("b", True), ("a", ("causes", {"b"}))]),
    ('switch "x" { "x" if b() => a(), "x" => c(), _ => false }',
     [("ab", True), ("c", True), ("b", ("causes", {"a"})), ("", ("causes", {"b", "c"}))]),
    ("let r = switch 2 { 1 => true }; r == () && a()", [("a", True)]),
    ('switch [1] { 1 => false, _ => a() }', [("a", True)]),
    ("switch -2 { -2 => a(), _ => false }", [("a", True)]),
    ("switch () { () => a(), _ => false }", [("a", True)]),
    # ??
    ("let x = (); (x ?? 7) == 7 && (5 ?? 7) == 5 && a()", [("a", True)]),
    ("let x = if false { 1 }; x ?? a()", [("a", True), ("", ("causes", {"a"}))]),
    # methods and built-ins on bool / int / string
    ('"abc".contains("b") && "abc".len() == 3 && "ab".starts_with("a") && "ab".ends_with("b") && a()',
     [("a", True)]),
    ('"héllo".len() == 5 && "".is_empty() && len("xy") == 2 && contains("xyz", "") && a()', [("a", True)]),
    ('type_of(1) == "i64" && type_of("x") == "string" && type_of([]) == "array" && type_of(()) == "()" '
     '&& type_of(true) == "bool" && a()', [("a", True)]),
    ('1 + "x" == "1x" && "x" + true == "xtrue" && "x" + () == "x" && (-5).to_string() == "-5" && a()',
     [("a", True)]),
    ("(42).to_string().len() == 2 && to_string(false) == \"false\" && a()", [("a", True)]),
    ('let s = ""; for i in range(0, 3) { s += i.to_string(); } s == "012" && a()', [("a", True)]),
    # loops, break / continue / return
    ("let n = 0; let i = 0; while i < 3 { i += 1; if i == 2 { continue; } n += i; } n == 4 && a()",
     [("a", True)]),
    ("let r = loop { break 5; }; r == 5 && a()", [("a", True)]),
    ("let i = 0; do { i += 1; } while i < 3; i == 3 && a()", [("a", True)]),
    ("let i = 0; do { i += 1; } until i >= 4; i == 4 && a()", [("a", True)]),
    ("let i = 0; do { i += 10; } while false; i == 10 && a()", [("a", True)]),
    ("let w = while false { }; w == () && a()", [("a", True)]),
    ("for (x, i) in [\"p\", \"q\"] { if i == 1 && x == \"q\" { return a(); } } false",
     [("a", True), ("", ("causes", {"a"}))]),
    ("let hits = 0; for m in [a(), b(), c()] { if !m { break; } hits += 1; } hits == 3",
     [("abc", True), ("ab", ("causes", {"c"}))]),
    ("let first = loop { if a() { break 1; } break 2; }; first == 1", [("a", True), ("", ("causes", {"a"}))]),
    # functions
    ("fn both(x, y) { x && y } both(a(), b())",  # arguments run eagerly: both members are called
     [("ab", True), ("b", ("causes", {"a"})), ("", ("causes", {"a", "b"}))]),
    ("fn fact(n) { if n <= 1 { 1 } else { n * fact(n - 1) } } fact(5) == 120 && a()", [("a", True)]),
    ("fn f() { a() } fn f(x) { x } f() && f(true)", [("a", True), ("", ("causes", {"a"}))]),
    ("fn g(x) { return x + 1; 0 } g(1) == 2 && a()", [("a", True)]),
    ("fn h(x) { let y = x; y += 1; y } let y = 5; h(y) == 6 && y == 5 && a()", [("a", True)]),
    ("fn a() { true } a() && b()", [("b", True), ("", ("causes", {"b"}))]),  # a script fn shadows member a
    # assignment and constants
    ('let x = 5; x = "s"; x == "s" && a()', [("a", True)]),
    ("const K = 2; let v = K * 3; v == 6 && a()", [("a", True)]),
    ("let x = 1; { let x = 2; x += 1; } x == 1 && a()", [("a", True)]),
    ("let x = 10; x -= 3; x *= 2; x /= 7; x %= 2; x |= 4; x &= 6; x ^= 1; x == 5 && a()", [("a", True)]),
    # numbers, strings, comments
    ("0x10 + 0o10 + 0b10 == 26 && 1_000 == 1000 && a()", [("a", True)]),
    ('"\\x41\\u00e9" == "Aé" && a() /* block /* nested */ comment */', [("a", True)]),
    # r06: rhai's standard packages (Engine::new()) — integers
    ("abs(-3) == 3 && (-3).abs() == 3 && abs(0) == 0 && a()", [("a", True)]),
    ("sign(-7) == -1 && sign(0) == 0 && (9).sign() == 1 && a()", [("a", True)]),
    ("is_zero(0) && !is_zero(5) && (-3).is_odd() && (4).is_even() && !(0).is_odd() && a()", [("a", True)]),
    ("max(3, 8) == 8 && min(3, 8) == 3 && max(-1, -1) == -1 && (2).min(-5) == -5 && a()", [("a", True)]),
    ('(255).to_hex() == "ff" && (8).to_octal() == "10" && (5).to_binary() == "101" && '
     '(-1).to_hex() == "ffffffffffffffff" && (0).to_binary() == "0" && a()', [("a", True)]),
    ('parse_int("42") == 42 && parse_int(" -17\t") == -17 && parse_int("+8") == 8 && parse_int("ff", 16) == 255 '
     '&& parse_int("-Z", 36) == -35 && parse_int("-9223372036854775808") == -9223372036854775807 - 1 && a()',
     [("a", True)]),
    ('if a() { true } else { parse_int("4x") == 4 }',
     [("a", True), ("", ("error", "Error parsing integer number '4x': invalid digit found in string"))]),
    ('if a() { true } else { parse_int(" ") == 0 }',
     [("", ("error", "Error parsing integer number ' ': cannot parse integer from empty string"))]),
    ('if a() { true } else { parse_int("9223372036854775808") == 0 }',
     [("", ("error", "number too large to fit in target type"))]),
    ('if a() { true } else { parse_int("-", 10) == 0 }', [("", ("error", "invalid digit found in string"))]),
    ('if a() { true } else { parse_int("1", 40) == 1 }', [("", ("error", "Invalid radix: '40'"))]),
    ("if a() { true } else { abs(-9223372036854775807 - 1) == 0 }", [("", ("error", "Negation overflow"))]),
    ('if a() { true } else { abs("x") == 1 }', [("", ("error", "Function not found: abs (string)"))]),
    # r06: ** (right-associative, binds tighter than *), << >> (tighter still), their compound forms
    ("2 ** 3 == 8 && 2 ** 3 ** 2 == 512 && -2 ** 2 == 4 && 2 * 3 ** 2 == 18 && 0 ** 0 == 1 && (-1) ** 7 == -1 && a()",
     [("a", True)]),
    ("1 << 2 == 4 && -8 >> 1 == -4 && 1 << 63 == -9223372036854775807 - 1 && 5 << -1 == 2 && -8 >> -2 == -32 && "
     "1 << 2 + 1 == 5 && 2 ** 1 << 2 == 16 && a()", [("a", True)]),  # (<< binds tighter than + and **)
    ("let x = 3; x **= 2; x <<= 1; x >>= 2; x == 4 && a()", [("a", True)]),
    ("if a() { true } else { 2 ** 63 == 0 }", [("", ("error", "Exponential overflow: 2 ** 63"))]),
    ("if a() { true } else { 2 ** -1 == 0 }", [("", ("error", "Integer raised to a negative index: 2 ** -1"))]),
    ("if a() { true } else { 1 << 64 == 0 }", [("", ("error", "Left-shift by too many bits: 1 << 64"))]),
    ("if a() { true } else { 1 >> -70 == 0 }", [("", ("error", "Left-shift by too many bits: 1 << 70"))]),
    ('if a() { true } else { "x" << 1 == 0 }', [("", ("error", "Function not found: << (string, i64)"))]),
    # strings
    ('"AbC".to_upper() == "ABC" && "AbC".to_lower() == "abc" && to_upper("\u00df") == "SS" && '
     '"\u0130".to_lower() == "i\u0307" && "\u00e9".to_upper() == "\u00c9" && a()', [("a", True)]),
    # Σ lowers to ς at the end of a word (Final_Sigma), else to σ; ' between letters is case-ignorable
    ('"\u039f\u0394\u039f\u03a3 \u03a3\u0391".to_lower() == "\u03bf\u03b4\u03bf\u03c2 \u03c3\u03b1" && '
     '"\u03a3".to_lower() == "\u03c3" && "A\u03a3\'".to_lower() == "a\u03c2\'" && '
     '"A\u03a3\'B".to_lower() == "a\u03c3\'b" && a()', [("a", True)]),
    # σ with no Σ among the literals: a run still reaches ς (σ -> Σ -> ς at the end of a word),
    # which must upper-case back to Σ
    ('let s = "a\u03c3"; s.to_upper().to_lower().to_upper() == s.to_upper() && s.to_upper().to_lower() != s && a()',
     [("a", True), ("", ("causes", {"a"}))]),
    ('let s = "Hello"; s.make_upper(); let t = "Hi"; make_lower(t); s == "HELLO" && t == "Hi" && a()',
     [("a", True)]),
    ('let s = "  x y \t"; s.trim(); let u = "\u00a0z\u3000"; u.trim(); s == "x y" && u == "z" && a()',
     [("a", True)]),
    ('let r = " x ".trim(); r == () && a()', [("a", True)]),  # trim changes its receiver, returns ()
    ('"hello".sub_string(1, 3) == "ell" && "hello".sub_string(-3, 2) == "ll" && "hello".sub_string(3) == "lo" && '
     '"h\u00e9llo".sub_string(1, 1) == "\u00e9" && "abc".sub_string(5, 1) == "" && "abc".sub_string(0, -1) == "" '
     '&& "abc".sub_string(-9, 2) == "ab" && sub_string("abc", 1) == "bc" && a()', [("a", True)]),
    ('let s = "hello"; s.crop(1, 3); let t = "hello"; t.crop(-2); let u = "abc"; u.crop(7); '
     's == "ell" && t == "lo" && u == "" && a()', [("a", True)]),
    ('"abcb".index_of("b") == 1 && "abcb".index_of("b", 2) == 3 && "abc".index_of("z") == -1 && '
     '"h\u00e9llo".index_of("l") == 2 && "abc".index_of("c", -1) == 2 && "abc".index_of("a", 5) == -1 && '
     '"".index_of("") == -1 && "ab".index_of("") == 0 && "ab".index_of("", 1) == 1 && a()', [("a", True)]),
    ('let s = "a-b-c"; s.replace("-", "+"); let t = "abc"; t.replace("", "."); let u = "aaa"; u.replace("aa", "b"); '
     's == "a+b+c" && t == ".a.b.c." && u == "ba" && a()', [("a", True)]),
    ('"a,b,,c".split(",") == ["a", "b", "", "c"] && " a b  c ".split() == ["a", "b", "c"] && '
     '"abc".split(1) == ["a", "bc"] && "abc".split(-1) == ["ab", "c"] && "abc".split(0) == ["abc", ""] && '
     '"a,b,c".split(",", 2) == ["a", "b,c"] && "a,b,c".split(",", 0) == ["a,b,c"] && '
     '"a,b,c".split_rev(",") == ["c", "b", "a"] && "a,b,c".split_rev(",", 2) == ["c", "a,b"] && '
     '"ab".split("") == ["", "a", "b", ""] && "aaa".split_rev("aa") == ["", "a"] && a()', [("a", True)]),
    ('"h\u00e9llo".bytes() == 6 && "h\u00e9llo".len() == 5 && a()', [("a", True)]),
    ('"ab".len == 2 && [1, 2, 3].len == 3 && "".is_empty && ![1].is_empty && "\u00e9".bytes == 2 && a()',
     [("a", True)]),  # the packages' property getters
    ('let s = "ab"; s.append(1); s.append(true); s.append(()); let t = "banana"; t.remove("an"); '
     'let u = "xyz"; u.truncate(2); let v = "q"; v.clear(); s == "ab1true" && t == "ba" && u == "xy" && v == "" && a()',
     [("a", True)]),
    ('"banana" - "an" == "ba" && "abc" - "" == "abc" && a()', [("a", True)]),
    ('let s = "aXbX"; s -= "X"; s == "ab" && a()', [("a", True)]),
    ('if a() { true } else { "abc".pop() == () }',
     [("", ("error", "unsupported by this engine: pop (string): it returns a character"))]),
    ('if a() { true } else { "abc".get(0) == () }', [("", ("error", "unsupported by this engine: get (string, i64)"))]),
    # arrays
    ("let v = [1, 2, 3]; let x = v.pop(); let y = v.shift(); x == 3 && y == 1 && v == [2] && [].pop() == () && a()",
     [("a", True)]),
    ("let v = [1, 3]; v.insert(1, 2); v.insert(-1, 9); v.insert(10, 4); v.insert(-10, 0); v == [0, 1, 2, 9, 3, 4] "
     "&& a()", [("a", True)]),
    ("let v = [1, 2, 3]; let r = v.remove(1); let z = v.remove(5); let w = v.remove(-1); let q = v.remove(-5); "
     "r == 2 && z == () && w == 3 && q == () && v == [1] && a()", [("a", True)]),
    ('let v = [3, 1, 2]; v.sort(); let w = ["b", "a", "B", "\u00e9"]; w.sort(); let b = [true, false]; b.sort(); '
     'let r = [1, 2, 3]; r.reverse(); let n = [[2], [1]]; n.sort(); '
     'v == [1, 2, 3] && w == ["B", "a", "b", "\u00e9"] && b == [false, true] && r == [3, 2, 1] && n == [[2], [1]] '
     '&& a()', [("a", True)]),
    ('if a() { true } else { let v = [1, "x"]; v.sort(); true }',
     [("", ("error", "sort() cannot be called with elements of different types"))]),
    ("let v = [1]; v.append([2, 3]); let w = [1, 2, 3, 4]; w.truncate(2); let x = [1, 2, 3, 4]; x.chop(1); "
     "let y = [1]; y.clear(); let z = [1, 2]; z.truncate(0); v == [1, 2, 3] && w == [1, 2] && x == [4] && y == [] "
     "&& z == [] && a()", [("a", True)]),
    ("let v = [1, 2, 3]; v.set(0, 9); v.set(7, 0); v.set(-1, 8); v.get(-1) == 8 && v.get(5) == () && "
     "v.get(-4) == () && v == [9, 2, 8] && a()", [("a", True)]),
    ("let v = [1, 2, 3, 4, 5]; let e = v.extract(1, 2); let t = v.extract(3); let d = v.drain(1, 2); "
     "e == [2, 3] && t == [4, 5] && d == [2, 3] && v == [1, 4, 5] && v.extract(0, 0) == [] && a()", [("a", True)]),
    ("let v = [1, 2, 3, 4, 5]; let r = v.retain(1, 3); let w = [1, 2]; let q = w.retain(0, 0); "
     "r == [1, 5] && v == [2, 3, 4] && q == [] && w == [1, 2] && a()", [("a", True)]),
    ('let v = [1, 2, 3]; v.splice(1, 1, ["x", "y"]); let w = []; w.splice(0, 3, [7]); let z = [1]; '
     'z.splice(5, 1, [2]); v == [1, "x", "y", 3] && w == [7] && z == [1, 2] && a()', [("a", True)]),
    ("let v = [1, 1, 2, 2, 1]; v.dedup(); let p = [1]; p.pad(3, 0); let s = [1, 2, 3, 4]; let t = s.split(1); "
     "v == [1, 2, 1] && p == [1, 0, 0] && s == [1] && t == [2, 3, 4] && [5, 6, 5].index_of(5, 1) == 2 && "
     "[5].index_of(7) == -1 && a()", [("a", True)]),
    ("let v = [1, 2]; pop(v); reverse(v); v == [1, 2] && a()", [("a", True)]),  # function style: copies
    ("let oks = [a(), b(), c()]; oks.dedup(); oks.len() == 1",
     [("abc", True), ("", True), ("ab", ("causes", {"c"})), ("a", ("causes", {"b", "c"}))]),
    ("let v = [a(), b()]; v.sort(); v[1]", [("a", True), ("b", True), ("", ("causes", {"a", "b"}))]),
    ('let n = 0; for p in "x,y,z".split(",") { if p == "y" && b() { n += 1; } } n == 1 && a()',
     [("ab", True), ("a", ("causes", {"b"}))]),
    ("if a() { true } else { [].pad(5000, 1) == [] }",
     [("", ("error", "engine limit: more than 16384 bytes of strings and arrays built"))]),
    # evaluation errors on some paths (500 for those requests)
    ("if a() { true } else { [1][5] == 1 }",
     [("a", True), ("", ("error", "Array index 5 out of bounds: only 1 element in array"))]),
    ("if a() { true } else { [][0] }", [("", ("error", "Array index 0 out of bounds: array is empty"))]),
    ("if a() { true } else { let x = 0; loop { x += 1; } }",
     [("a", True), ("", ("error", "engine limit: more than 100000 loop iterations"))]),
    ("fn f(n) { f(n + 1) } if a() { true } else { f(0) }", [("a", True), ("", ("error", "Stack overflow"))]),
    ('if a() { true } else { "x".len() + "y" }',
     [("", ("error", "did not evaluate to a boolean: Output type incorrect: string (expecting bool)"))]),
    ("if a() { true } else { let s = \"x\"; loop { s += s; } }",
     [("", ("error", "engine limit: more than 16384 bytes of strings and arrays built"))]),
    ("if a() { true } else { 5[0] }", [("", ("error", "Indexer unavailable: i64"))]),
    ('if a() { true } else { [1]["0"] }', [("", ("error", "Array index must be an i64, found string"))]),
    ("if a() { true } else { for x in 5 { } }", [("", ("error", "For loop expects an iterable type, found i64"))]),
    ("if a() { true } else { 1 in \"abc\" }", [("", ("error", "Function not found: contains (string, i64)"))]),
    ('if a() { true } else { "x" in 1..3 }', [("", ("error", "Function not found: contains (range, string)"))]),
    ("if a() { true } else { len(5) == 1 }", [("", ("error", "Function not found: len (i64)"))]),
    ("if a() { true } else { while 1 { } }",
     [("", ("error", "Boolean value expected for the while condition, found i64"))]),
    ("if a() { true } else { switch 1 { 1 if 2 => true, _ => false } }",
     [("", ("error", "Boolean value expected for the switch case condition, found i64"))]),
    ("if a() { true } else { a(1) }", [("", ("error", "Function not found: a (i64)"))]),
    ("if a() { true } else { let z = " + "[" * 18 + "1" + "]" * 18 + "; z == z }",
     [("", ("error", "engine limit: arrays nested more than 16 deep"))]),
    ("if a() { true } else { [1, 2].to_string() == \"\" }",
     [("", ("error", "unsupported by this engine: converting an array to a string"))]),
    ("if a() { true } else { \"ab\"[0] == 1 }",
     [("", ("error", "unsupported by this engine: indexing a string (characters)"))]),
]

INVALID = [
    ("a() && 1.5 > 1", "unsupported by this engine: floating-point numbers"),
    ("let m = #{x: 1}; a()", "unsupported by this engine: object maps"),
    ("'c' == 'c' && a()", "unsupported by this engine: character literals"),
    ("`x${1}` == \"x1\" && a()", "unsupported by this engine: back-tick strings"),
    ("let f = |x| x + 1; a()", "unsupported by this engine: closures"),
    ("let r = 1..3; a()", "unsupported by this engine: range values outside `for` and `in`"),
    ("let r = range(1, 3); a()", "unsupported by this engine: range values outside `for` and `in`"),
    ("for i in range(0, 9, 2) {} a()", "unsupported by this engine: range() with a step"),
    ("\"ab\".size == 2 && a()", "unsupported by this engine: property access (.size)"),
    ("throw \"x\"; a()", "unsupported by this engine: throw"),
    ("print(1); a()", "unsupported by this engine: print"),
    ("a() && [1, 2].to_string() == \"[1, 2]\"", "unsupported by this engine: converting an array to a string"),
    ("for c in \"ab\" { } a()", "unsupported by this engine: iterating over a string (characters)"),
    ("let a1 = [[1]]; a1[0][0] = 2; a()", "unsupported by this engine: assigning to a nested index"),
    ("const K = 1; K = 2; a()", "Syntax error: cannot assign to the constant 'K'"),
    ("break; a()", "Syntax error: break should only be used inside a loop"),
    ("switch 1 { 1 => a(), 1 => b() }", "Syntax error: duplicated switch case"),
    ("switch 1 { _ => a(), 1 => b() }", "Syntax error: the wildcard case '_' must be the last case"),
    ("if true { fn f() { 1 } } a()", "Syntax error: functions can only be defined at global level"),
    ("fn f(x) { x } fn f(y) { y } a()", "Syntax error: function 'f' with 1 parameters is defined more than once"),
    ("let x = 1; x.push(2); a()", "Function not found: push (i64, i64)"),
    # r06: the standard packages' functions outside the engine are refused by name at load
    ("sqrt(4) == 2 && a()", "unsupported by this engine: sqrt"),
    ("let f = 1; [1].filter(f) == [] && a()", "unsupported by this engine: filter"),
    ("timestamp() == () || a()", "unsupported by this engine: timestamp"),
    ('"ab".chars() == [] && a()', "unsupported by this engine: chars"),
    ("(5).get_bit(1) && a()", "unsupported by this engine: get_bit"),
    ("const V = [1]; V.pop(); a()", "Syntax error: cannot assign to the constant 'V'"),
    ("let v = [[1]]; v[0].sort(); a()", "unsupported by this engine: mutating an element in place (x[i].sort(..))"),
    ('parse_int("z") == 0 && a()', "Error parsing integer number 'z': invalid digit found in string"),
    ("nope(1, 2) || a()", "Function not found: nope (i64, i64)"),
    ("let s = 0; for i in 0..200000 { s += 1; } a()", "engine limit: more than 100000 loop iterations"),
    ("99999999999999999999 > 1", "Syntax error: integer literal too large"),
    ("0xZZ > 1", "Syntax error: invalid number: 0xZZ"),
]
