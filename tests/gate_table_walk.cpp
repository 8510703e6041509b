// Walks csrc/gates.h for tests/test_gate_table.py: the arguments are
// (kind, p0, p1, p2) quadruples; prints one JSON object per quadruple with
// the kind's serializer id both ways and gate_shape's numbers.  A stand-alone
// host program, so it is also what -fsanitize=address,undefined runs on.
#include <stdio.h>
#include <stdlib.h>
#include "../qp-zk-circuits-rm_amd/csrc/gates.h"

int main(int argc, char **argv) {
  printf("[");
  for (int i = 1; i + 3 < argc; i += 4) {
    const uint32_t kind = (uint32_t)strtoul(argv[i], nullptr, 10);
    const uint64_t p0 = strtoull(argv[i + 1], nullptr, 10), p1 = strtoull(argv[i + 2], nullptr, 10),
                   p2 = strtoull(argv[i + 3], nullptr, 10);
    const qg::GateShape s = qg::gate_shape(kind, p0, p1, p2);
    const uint32_t serial = kind < qg::G_NKINDS ? qg::serial_id((qg::GateKind)kind) : ~0u;
    printf("%s\n{\"serial_id\": %u, \"kind_from_serial\": %u, \"serial_params\": %u, \"ok\": %s, \"wires\": %llu, "
           "\"consts\": %llu, \"constraints\": %llu, \"degree\": %u}",
           i > 1 ? "," : "", serial, (unsigned)qg::kind_from_serial(serial),
           kind < qg::G_NKINDS ? qg::serial_params((qg::GateKind)kind) : 0u, s.ok ? "true" : "false",
           (unsigned long long)s.wires, (unsigned long long)s.consts, (unsigned long long)s.constraints, s.degree);
  }
  printf("\n]\n");
  return 0;
}
