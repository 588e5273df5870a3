// Stand-in gtsam/linear/HessianFactor.h for tests/cpp/test_plane_ba_drop_in.cpp: the one of tests/cpp/glim_standin (the 1- and 2-key
// constructors, same members) plus the N-key constructor of GTSAM the bundle-adjustment factors need.  This directory goes IN FRONT of
// glim_standin on the include path; everything else comes from there.
#pragma once
#include <gtsam/base/Matrix.h>
#include <gtsam/inference/Key.h>
#include <map>
#include <memory>
#include <vector>
namespace gtsam {
class GaussianFactor {
public:
  typedef std::shared_ptr<GaussianFactor> shared_ptr;
  virtual ~GaussianFactor() {}
  std::map<Key, Matrix> hessianBlockDiagonal() const;
};
class HessianFactor : public GaussianFactor {
public:
  // error(x) = 0.5 (f - 2 x^T g + x^T G x)
  HessianFactor(Key j, const Matrix& G, const Vector& g, double f) : keys_{j}, G22_(G), g2_(g), f_(f) {}
  HessianFactor(Key j1, Key j2, const Matrix& G11, const Matrix& G12, const Vector& g1, const Matrix& G22, const Vector& g2, double f)
  : keys_{j1, j2}, G11_(G11), G12_(G12), G22_(G22), g1_(g1), g2_(g2), f_(f) {}
  // GTSAM's N-key form: Gs holds the upper block triangle row by row (G11, G12, .., G1n, G22, ..), gs one block per key
  HessianFactor(const KeyVector& js, const std::vector<Matrix>& Gs, const std::vector<Vector>& gs, double f) : keys_(js), Gs_(Gs), gs_(gs), f_(f) {}
  KeyVector keys_;
  Matrix G11_, G12_, G22_;
  Vector g1_, g2_;
  std::vector<Matrix> Gs_;
  std::vector<Vector> gs_;
  double f_ = 0.0;
};
class GaussianFactorGraph {
public:
  std::map<Key, Matrix> hessianBlockDiagonal() const;
};
}  // namespace gtsam
