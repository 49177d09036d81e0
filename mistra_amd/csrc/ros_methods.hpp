// The five Rosenbrock methods of Rosenbrock_x (gas.f:1514-1895 | aer.f | tot.f) as compile-time tables: what the method kernels
// (ros3_kernel.hip: ros3_integrate_kernel<MT, NT, 3, METHOD>) are compiled with and what mistra_chem_method_table hands to the host.
// Values typed in as data from Ros2_x .. Rodas4_x; ros_Alpha stands in a table of its own (below): FunTemplate_x ignores T, only the kernels whose rate
// constants are linear in time read it.  Plain C++: host and device.
#pragma once

namespace mistra {

// IPAR(4) of Rosenbrock_x (gas.f:1057-1077); 0 selects Ros4
enum RosMethodId : int { kRos2 = 1, kRos3 = 2, kRos4 = 3, kRodas3 = 4, kRodas4 = 5 };

struct RosMethodTable {
  int S;                 // ros_S: stages
  double A[15], C[15];   // strictly lower triangular, row-wise: A(i,j) = ros_A((i-1)*(i-2)/2 + j)
  double M[6], E[6];     // new solution, error estimator
  double Gamma[6];
  bool NewF[6];          // stage i evaluates the function anew (else it reuses the one of stage i-1)
  double ELO;            // estimator of local order
};

// SQRT(2.0d0), correctly rounded; Ros2_x forms g = 1 + 1/SQRT(2) from it at run time (gas.f:1529)
constexpr double kRosSqrt2 = 1.4142135623730951;

constexpr RosMethodTable ros_method_table(int method) {
  switch (method) {
    case kRos2: {      // gas.f:1529-1563, the reference's own expressions
      constexpr double g = 1.0 + 1.0 / kRosSqrt2;
      return RosMethodTable{2,
                            {(1.0) / g},
                            {(-2.0) / g},
                            {(3.0) / (2.0 * g), (1.0) / (2.0 * g)},
                            {1.0 / (2.0 * g), 1.0 / (2.0 * g)},
                            {g, -g},
                            {true, true},
                            2.0};
    }
    case kRos3:        // gas.f:1596-1626
      return RosMethodTable{3,
                            {1.0, 1.0, 0.0},
                            {-0.10156171083877702091975600115545e+01, 0.40759956452537699824805835358067e+01, 0.92076794298330791242156818474003e+01},
                            {0.1e+01, 0.61697947043828245592553615689730e+01, -0.42772256543218573326238373806514e+00},
                            {0.5e+00, -0.29079558716805469821718236208017e+01, 0.22354069897811569627360909276199e+00},
                            {0.43586652150845899941601945119356e+00, 0.24291996454816804366592249683314e+00, 0.21851380027664058511513169485832e+01},
                            {true, true, false},
                            3.0};
    case kRos4:        // gas.f:1667-1708
      return RosMethodTable{4,
                            {0.2000000000000000e+01, 0.1867943637803922e+01, 0.2344449711399156e+00, 0.1867943637803922e+01, 0.2344449711399156e+00, 0.0},
                            {-0.7137615036412310e+01, 0.2580708087951457e+01, 0.6515950076447975e+00, -0.2137148994382534e+01, -0.3214669691237626e+00,
                             -0.6949742501781779e+00},
                            {0.2255570073418735e+01, 0.2870493262186792e+00, 0.4353179431840180e+00, 0.1093502252409163e+01},
                            {-0.2815431932141155e+00, -0.7276199124938920e-01, -0.1082196201495311e+00, -0.1093502252409163e+01},
                            {0.5728200000000000e+00, -0.1769193891319233e+01, 0.7592633437920482e+00, -0.1049021087100450e+00},
                            {true, true, true, false},
                            4.0};
    case kRodas3:      // gas.f:1739-1781
      return RosMethodTable{4,
                            {0.0, 2.0, 0.0, 2.0, 0.0, 1.0},
                            {4.0, 1.0, -1.0, 1.0, -1.0, -(8.0 / 3.0)},
                            {2.0, 0.0, 1.0, 1.0},
                            {0.0, 0.0, 0.0, 1.0},
                            {0.5, 1.5, 0.0, 0.0},
                            {true, false, true, true},
                            3.0};
    case kRodas4:      // gas.f:1820-1892
      return RosMethodTable{6,
                            {0.1544000000000000e+01, 0.9466785280815826e+00, 0.2557011698983284e+00, 0.3314825187068521e+01, 0.2896124015972201e+01,
                             0.9986419139977817e+00, 0.1221224509226641e+01, 0.6019134481288629e+01, 0.1253708332932087e+02, -0.6878860361058950e+00,
                             0.1221224509226641e+01, 0.6019134481288629e+01, 0.1253708332932087e+02, -0.6878860361058950e+00, 1.0},
                            {-0.5668800000000000e+01, -0.2430093356833875e+01, -0.2063599157091915e+00, -0.1073529058151375e+00, -0.9594562251023355e+01,
                             -0.2047028614809616e+02, 0.7496443313967647e+01, -0.1024680431464352e+02, -0.3399990352819905e+02, 0.1170890893206160e+02,
                             0.8083246795921522e+01, -0.7981132988064893e+01, -0.3152159432874371e+02, 0.1631930543123136e+02, -0.6058818238834054e+01},
                            {0.1221224509226641e+01, 0.6019134481288629e+01, 0.1253708332932087e+02, -0.6878860361058950e+00, 1.0, 1.0},
                            {0.0, 0.0, 0.0, 0.0, 0.0, 1.0},
                            {0.2500000000000000e+00, -0.1043000000000000e+00, 0.1035000000000000e+00, -0.3620000000000023e-01, 0.0, 0.0},
                            {true, true, true, true, true, true},
                            4.0};
  }
  return RosMethodTable{0, {}, {}, {}, {}, {}, {}, 0.0};
}

template <int METHOD>
inline constexpr RosMethodTable kRosMethod = ros_method_table(METHOD);

// ros_Alpha of the same five routines: stage i evaluates the function at T + ros_Alpha(i)*Direction*H.  A table of its own, read by the kernels whose
// rate constants depend on the time (ros3_kernel.hip: VARIANT 10) and by nothing else: RosMethodTable keeps the layout mistra_chem_method_table hands out.
struct RosAlphaTable {
  double Alpha[6];
};
constexpr RosAlphaTable ros_alpha_table(int method) {
  switch (method) {
    case kRos2: return RosAlphaTable{{0.0, 1.0}};
    case kRos3: return RosAlphaTable{{0.0, 0.43586652150845899941601945119356e+00, 0.43586652150845899941601945119356e+00}};
    case kRos4: return RosAlphaTable{{0.0, 0.1145640000000000e+01, 0.6552168638155900e+00, 0.6552168638155900e+00}};
    case kRodas3: return RosAlphaTable{{0.0, 0.0, 1.0, 1.0}};
    case kRodas4: return RosAlphaTable{{0.0, 0.386, 0.21, 0.63, 1.0, 1.0}};
  }
  return RosAlphaTable{{}};
}
template <int METHOD>
inline constexpr RosAlphaTable kRosAlpha = ros_alpha_table(METHOD);

// whether stage i + 1 (i >= 1) works on a function value formed in this step's stages 2 .. i + 1, not on Fcn0 (gas.f:1247-1262)
constexpr bool ros_fresh_fcn(int method, int i) {
  const RosMethodTable t = ros_method_table(method);
  bool any = false;
  for (int s = 1; s <= i; s++) any = any || t.NewF[s];
  return any;
}

}  // namespace mistra
