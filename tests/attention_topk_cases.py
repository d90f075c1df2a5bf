"""The case table of the top-k read-out tests (tests/test_attention_topk_cpu.py, tests/test_attention_topk_gpu.py):
tests/attention_mass_cases.py's shapes, inputs and lens patterns - T = 2, H = 2, d = 16, m 16 and 40, Nq either side of the 16-row
tile, Nc at the edges of every form (keys 1, 31, 32 | long 33, 64, 255, 256 | paged 257, 512, 513) - each with k = 1, 3 and 16: one
entry, a few, and the kernels' most, which exceeds lens[t] and Nc in the small cases (the padding rule).  One more paged case keeps
513 shots in 1024 slots."""
from tests import attention_mass_cases as MC

T, H, D = MC.T, MC.H, MC.D
NQS, NQ = MC.NQS, MC.NQ
KS = [1, 3, 16]
CASES = list(MC.CASES)                          # (form, Nc, m, lens)
WIDE = ("paged", 513, 40, (510, 513), 1024)     # form, shots, m, lens, capacity
inputs, proj, valid, poisoned, case_id, EDGE = MC.inputs, MC.proj, MC.valid, MC.poisoned, MC.case_id, MC.EDGE
