// What csrc/group_regression.hip and csrc/group_regression_vx.hip share beside the solves of csrc/regression_solve.h: the layout of the
// prepared block.  (The epilogue of a row, which they share too, is a body: csrc/regression_epilogue_body.h.)
#pragma once
#include "cohort.h"
#include "regression_solve.h"

namespace oai {

// the prepared block of "Cohort regression"; "Vertex-wise design columns" appends its own arrays to it
struct Prepared {
    double *R, *Q, *mean;
    int* n;
    unsigned char* ok;
    size_t bytes;
    Prepared(const void* base, long long N, long long V) {
        Ws ws(base);
        R = ws.take<double>((size_t)(N * V));
        Q = ws.take<double>((size_t)V);
        mean = ws.take<double>((size_t)V);
        n = ws.take<int>((size_t)V);
        ok = ws.take<unsigned char>((size_t)V);
        bytes = ws.off;
    }
};

}  // namespace oai
