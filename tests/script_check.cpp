// script_check.cpp — the wide path's group programs (policy-server_amd/csrc/groupvm.hpp) alone on the
// host, as a plain executable for AddressSanitizer and UBSan (tests/test_script_vm.py builds and runs
// it; no Python in this process). Every script of the input file is compiled for the wide path
// (expr.cpp, force_wide) and run for every vector of member results: the script form through
// run_script_prog with its scratch a heap block of exactly run_script_words(prog) words, wide jump
// code through run_wide_prog with a bit stack of exactly `depth` bits, the program bytes a heap block
// of exactly their length — so a step past the stack, the variables, the frames, the arena or the
// program is the sanitizer's to catch. Each run must agree with the host interpreter
// (GroupProgram::run): an error gives 2, a bool 1 / 0, and a false result hands `cause` exactly the
// called members that rejected.
//
// Input: "<count>\n", then per script "<members> <bytes>\n<member names>\n<script bytes>\n".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "expr.hpp"
#include "groupvm.hpp"

using namespace kw;

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: script_check <scripts file>\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  size_t count = 0;
  if (!(in >> count)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  size_t vm = 0, wide = 0, refused = 0, runs = 0, failures = 0;
  for (size_t k = 0; k < count; ++k) {
    size_t nmem = 0, len = 0;
    in >> nmem >> len;
    std::vector<std::string> members(nmem);
    for (std::string& m : members) in >> m;
    in.get();  // the newline after the names
    std::string expr(len, '\0');
    in.read(&expr[0], (std::streamsize)len);
    if (!in || nmem > 16) {
      fprintf(stderr, "bad record %zu\n", k);
      return 2;
    }
    const GroupProgram g = compile_group_expression(expr, members, /*force_wide=*/true);
    if (!g.valid || g.eval_error || !g.wide) {  // (refused at load: nothing for the wide path to run)
      ++refused;
      continue;
    }
    ++(g.script ? vm : wide);
    std::unique_ptr<uint8_t[]> prog(new uint8_t[g.code.size()]);
    memcpy(prog.get(), g.code.data(), g.code.size());
    const size_t words = g.script ? (size_t)run_script_words(prog.get()) : (g.depth + 63u) / 64u;
    for (uint32_t mask = 0; mask < (1u << nmem); ++mask) {
      auto ok = [mask](uint32_t m) { return ((mask >> m) & 1u) != 0; };
      const ExprOutcome ref = g.run(ok);
      uint32_t want_causes = 0, causes = 0;
      for (uint32_t m : ref.called)
        if (!ok(m)) want_causes |= 1u << m;
      auto cause = [&causes](uint32_t m) { causes |= 1u << m; };
      std::unique_ptr<uint64_t[]> scratch(new uint64_t[words]);
      memset(scratch.get(), 0xA5, words * sizeof(uint64_t));  // (a run reads nothing it has not written)
      const int got = g.script ? run_script_prog(prog.get(), scratch.get(), ok, cause)
                               : (run_wide_prog(prog.get(), (uint32_t)g.code.size(), scratch.get(), ok, cause) ? 1 : 0);
      const int want = ref.error ? 2 : ref.value ? 1 : 0;
      ++runs;
      if (got != want || (want == 0 && causes != want_causes)) {
        ++failures;
        fprintf(stderr, "script %zu mask %u: got %d causes %x, the interpreter %d causes %x (%s)\n  %s\n", k, mask, got,
                causes, want, want_causes, ref.message.c_str(), expr.c_str());
      }
    }
  }
  printf("scripts %zu vm %zu wide %zu refused %zu runs %zu failures %zu\n", count, vm, wide, refused, runs, failures);
  return failures ? 1 : 0;
}
