// eaqhm_modify_shape.inc — compiles eaqhm_modify_body.inc once more under the MAP_* macros in force, with the
// shape-invariant phase term of DESIGN.md §11 switched on, and switches it off again.  Included by eaqhm_modify.hip
// after each variant's own inclusion of the body.  No include guard: included once per variant.
#undef EAQHM_MODIFY_SHAPE
#undef SHAPE_WEIGHT
#undef SHAPE_INIT
#undef SHAPE_ADD
#undef SHAPE_SAMPLE
#define EAQHM_MODIFY_SHAPE 1
#define SHAPE_WEIGHT(g) 1.0
#define SHAPE_SS ((double*)(ccode + (((size_t)NR * K + 7) & ~(size_t)7)) + (size_t)NR * MAP_CROW)   // [TBS]
#define SHAPE_INIT
#define SHAPE_SAMPLE                                                                                                \
  SHAPE_SS[s] = (j < A.No_ti - 1) ? shape_advance(Sh, j, r, (MAP_G) - 1.0, D, A.fs) : Sh.S[A.No_ti - 1];
#define SHAPE_ADD                                                                                                   \
  {                                                                                                                 \
    const double shs = SHAPE_SS[s];                                                                                 \
    for (int k = g; k < K; k += G) X[(size_t)k * TP + s] += (2.0 * M_PI * (double)(k + 1)) * shs;                   \
  }
#include "eaqhm_modify_body.inc"
#undef SHAPE_SS
#undef EAQHM_MODIFY_SHAPE
#undef SHAPE_WEIGHT
#undef SHAPE_INIT
#undef SHAPE_ADD
#undef SHAPE_SAMPLE
#define EAQHM_MODIFY_SHAPE 0
#define SHAPE_WEIGHT(g) g
#define SHAPE_INIT
#define SHAPE_ADD
#define SHAPE_SAMPLE
