"""Inputs of the tests of the scene batches' gravity from located vision: tests/test_scenes_located_cpu.py,
tests/test_gpu_scenes_located.py.

TEST INFRASTRUCTURE.  Every batch the GPU file steps is drawn by scenes_seen_cases.batch from a row (seed, n, width, scale, scenes):
scene s is the reference's initial state of n bodies for seed + s, its positions multiplied by `scale`.  The rows are those of
tests/scenes_seen_cases.py where they hold this step's premises, which ask more than the seen step's -- some member must be nearest at
one depth on several columns, so that L1's tie rule decides a column --, and other seeds or scales, found on the CPU by
tests/test_scenes_located_cpu.py's own figures, where they do not.  A blind body, a seeing majority and a step that differs from
coasting and from nb_step's are held by every scene of a row; several members in some eye and a tie in some member by every row (a
tie is rare at 64 columns: 1 to 3 seeds in a hundred have one at scale 0.3, so no three consecutive seeds all have).  Rows of fewer than PREMISE_MIN_N bodies or narrower than
PREMISE_MIN_WIDTH columns cannot hold the premises and are compared for equality alone."""
from scenes_seen_cases import F, PREMISE_MIN_N, PREMISE_MIN_WIDTH, UP, batch, holds_premises  # noqa: F401  (the tests' K.*)

# (seed, n, width, scale, scenes): the sizes on both sides of every line the launcher draws (one wave per eye up to 128 bodies, four
# above; a second pass over the bodies above 64 / 256), three scenes each (B = 1 takes the first), two at n = 2 048
SIZES = {n: (1100, n, 1024, 1.0, 3) for n in (1, 2, 3, 63, 64, 65, 100, 128, 129, 257)}
SIZES[64] = (1101, 64, 1024, 1.0, 3)         # (seed 1100 at n = 64 has no member that ties)
SIZES[2048] = (5, 2048, 1024, 1.0, 2)
# widths at n = 65: below, at and above a wave's 64 columns, no power of two, the maximum; narrow rows look at a scene drawn together
# (at scale 0.1 no narrow row of seeds 1100 .. 1199 has a tie; at 0.3 a few seeds have, and these triples hold the rest as well)
WIDTHS = {1: (1100, 65, 1, 0.1, 3), 63: (1120, 65, 63, 0.3, 3), 64: (1120, 65, 64, 0.3, 3), 65: (1120, 65, 65, 0.3, 3),
          1000: (1100, 65, 1000, 1.0, 3), 4096: (1100, 65, 4096, 1.0, 3)}
# SL3: the lists
LISTS = {(n, 1024): (1100, n, 1024, 1.0, 3) for n in (64, 100, 129)}
LISTS[(64, 1024)] = SIZES[64]
LISTS.update({(64, 64): (1177, 64, 64, 0.3, 3), (100, 64): (1178, 100, 64, 0.3, 3), (129, 64): (1100, 129, 64, 0.3, 3)})
FLOOR = (1100, 100, 1024, 1.0, 64)
ROWS = list(SIZES.values()) + list(WIDTHS.values()) + list(LISTS.values()) + [FLOOR]
