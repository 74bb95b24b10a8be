// jacobi.h -- the host eigen-solver the estimation drivers share (defined in lda.cc; feanorm.cc takes it for the PCA).
#pragma once
#include <vector>

namespace aasr {

// Cyclic Jacobi on the symmetric n x n row-major matrix a: on return a's diagonal holds the eigenvalues and the
// COLUMNS of v the eigenvectors, in no particular order.
void jacobi_eigen(std::vector<double> &a, int n, std::vector<double> &v);

}  // namespace aasr
