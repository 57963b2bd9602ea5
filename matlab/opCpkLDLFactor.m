classdef opCpkLDLFactor < opSpot
%OPCPKLDLFACTOR  M' and conj(M) of an opCpkLDL2: the bare factor composite
%                P*inv(L')*inv(D)*inv(L)*P' that opLDL2 returns there (ops/opLDL2.m:127-136).
%
%   F = opCpkLDLFactor(h, n) applies the factors the cpkHandle h owns (the handle is shared with
%   the opCpkLDL2 it came from, which keeps the device factorization alive for both).  F*x is
%   one LDL solve: no refinement, no residual update, none of M's properties.  F*X with an
%   n-by-k matrix solves all k columns in one call (cpk_mex 'pc_apply_ldl'): the device streams
%   the factor once per panel of 8 columns, and each column equals F*X(:,j) bit for bit.
%   The composite is real and symmetric, so F.' , F' and conj(F) are F.

   properties( SetAccess = private )
      h             % cpkHandle shared with the opCpkLDL2
   end

   methods
      function op = opCpkLDLFactor(h, n)
         if nargin ~= 2
            error('Invalid number of arguments.');
         end
         op = op@opSpot('CpkLDLFactor', n, n);
         op.h = h;
         op.sweepflag = true;   % multiply takes the whole block
      end

      function opOut = transpose(op)
         opOut = op;
      end
      function opOut = ctranspose(op)
         opOut = op;
      end
      function opOut = conj(op)
         opOut = op;
      end
      % double: a plain product, so op * eye(n) is legal here (it is not for opLDL2 itself)
      function x = double(op)
         x = op * eye(op.n);
      end
   end

   methods( Access = protected )
      function y = multiply(op, x, mode) %#ok<INUSD>
         y = cpk_mex('pc_apply_ldl', op.h.id, full(x));
      end
   end
end
