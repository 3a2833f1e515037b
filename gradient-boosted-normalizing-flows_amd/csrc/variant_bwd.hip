// One translation unit per backward-kernel variant of the training path: -DGBNF_V_ARGS="KIND,HT,OT,ACTA,ACTB,DEPTH" [-DGBNF_V_SAFE=1: bf16x6]
#include "gbnf_train_bwd.hip.h"
#ifndef GBNF_V_ARGS
#error "compile with -DGBNF_V_ARGS=KIND,HT,OT,ACTA,ACTB,DEPTH"
#endif
#ifdef GBNF_V_SAFE
#define GBNF_V_PREC 1
#else
#define GBNF_V_PREC 0
#endif
#define GBNF_INST2(...) GBNF_INSTANTIATE_HX3_BWD(__VA_ARGS__)
GBNF_INST2(GBNF_V_PREC, GBNF_V_ARGS)
