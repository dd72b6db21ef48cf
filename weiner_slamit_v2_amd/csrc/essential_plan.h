// essential_plan.h — the choice of edges of Optimizer::OptimizeEssentialGraph (ORB_SLAM2/src/Optimizer.cc:847-983) over slot-numbered
// tables, and the incidence lists the device assembles H and b from.  Host only, plain C++17, no HIP include: tests/test_essential_plan.py
// builds essential_plan.cc with g++ (and a stand-alone driver under -fsanitize=address,undefined).  include/slamit.h
// (slamit_essential_plan) states what is kept of the reference and what departs from it.
#ifndef SLAMIT_ESSENTIAL_PLAN_H
#define SLAMIT_ESSENTIAL_PLAN_H
#include <stdint.h>

#include <vector>

#include "../../include/slamit.h"

struct EgEdge { int32_t v0, v1, kind; };

// The tables themselves: counts, CSR pointer arrays that ascend from 0, every slot inside [0, n_kf) (parents: -1 too), ord_n within
// row_cap.  SLAMIT_OK, or SLAMIT_ERR_ARG with *why naming the first offence.
int eg_check_graph(const slamit_eg_graph& g, const char** why);

// The edge list in the reference's insertion order (g has passed eg_check_graph).  SLAMIT_ERR_ARG when an edge names a bad keyframe.
int eg_plan_edges(const slamit_eg_graph& g, std::vector<EgEdge>& edges, const char** why);

// An edge list as a caller hands it to the optimisation: endpoints inside [0, n_kf), on good keyframes, distinct; kinds known.
int eg_check_edges(int32_t n_kf, const uint8_t* bad, int32_t n_edge, const int32_t* v0, const int32_t* v1, const int32_t* kind, const char** why);

// inc_ptr[n_kf + 1], inc_edge[2 n_edge]: per slot its incident edges in list order, entry = 2 * edge + side (side 1: the slot is v1).
void eg_incidence(int32_t n_kf, int32_t n_edge, const int32_t* v0, const int32_t* v1, int32_t* inc_ptr, int32_t* inc_edge);

// An incidence table a caller supplies (the device form cannot be shown one first, the host form can): exactly what eg_incidence gives.
bool eg_incidence_matches(int32_t n_kf, int32_t n_edge, const int32_t* v0, const int32_t* v1, const int32_t* inc_ptr, const int32_t* inc_edge);

#endif
