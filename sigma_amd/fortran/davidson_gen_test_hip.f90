!==========================================================================!
! davidson_gen_test_hip: the smallest eigenpairs of K x = lambda M x        !
! through the stand-alone host layer.  The 1-D P1 pair on 127 interior      !
! nodes, h = 1/128: K = (1/h) tridiag(-1, 2, -1), M = (h/6) tridiag(1, 4,   !
! 1), whose eigenvalues are 6 (1 - c_j) / (h^2 (2 + c_j)), c_j = cos(j pi   !
! h).  hip_davidson_gen for 4 pairs with hip_jacobi() set up on K, ncv = 20 !
! and tol = 1e-8 from the default start vector.  Every lambda_i must lie    !
! within |r_i|_2 / sqrt(lambda_min(M)) of the i-th closed-form value, r_i   !
! the residual K v - lambda M v this program forms itself (the residual     !
! theorem in the M-inner product with |v|_M = 1, lambda_min(M) >= h/3 by    !
! Gershgorin), plus n eps 12/h^2 for the roundings.                         !
!==========================================================================!
program davidson_gen_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nn = 127, k = 4
    real(dp), parameter :: pi = 3.14159265358979323846264338327950288_dp
    real(dp), parameter :: h = 1.0_dp / real(nn + 1, dp)
    type(hip_csr_matrix), target :: A, B
    type(hip_linear_solver), pointer :: pc
    real(dp), allocatable :: V(:,:), q(:), p(:), val(:)
    integer, allocatable :: ptr(:), node(:)
    real(dp) :: lambda(k), resid(k), exact(k), own, bar, c
    integer :: i, j, e, fails, steps, products, products_b, applies, restarts, found
    logical :: converged

    fails = 0
    call hip_check(sgm_init(0_c_int))
    allocate(V(nn, k), q(nn), p(nn), val(3 * nn), ptr(nn + 1), node(3 * nn))
    call tridiag(A, -1.0_dp / h, 2.0_dp / h)
    call tridiag(B, h / 6.0_dp, 4.0_dp * h / 6.0_dp)
    do j = 1, k
        c = cos(real(j, dp) * pi * h)
        exact(j) = 6.0_dp * (1.0_dp - c) / (h * h * (2.0_dp + c))
    enddo

    pc => hip_jacobi()
    call pc%setup(A)
    call hip_davidson_gen(A, B, k, lambda, pc=pc, V=V, resid=resid, ncv=20, tol=1.0e-8_dp, max_steps=20000, steps=steps, &
        & products=products, products_b=products_b, applies=applies, restarts=restarts, found=found, converged=converged)
    call check('davidson_gen: converged with 4 pairs', converged .and. found == k)
    call check('davidson_gen: products with A = 1 + steps + pairs', products == 1 + steps + k)
    call check('davidson_gen: products with B = 1 + steps + pairs', products_b == 1 + steps + k)
    call check('davidson_gen: one apply per step', applies == steps)
    print '(a,i0,a,i0,a,i0,a,i0,a,i0)', ' DAVIDSON_GEN steps ', steps, ' products ', products, ' products_b ', products_b, &
        & ' applies ', applies, ' restarts ', restarts
    do i = 1, k
        call A%matvec(V(:, i), q)
        call B%matvec(V(:, i), p)
        own = sqrt(sum((q - lambda(i) * p)**2))
        bar = max(own, resid(i)) / sqrt(h / 3.0_dp) + real(nn, dp) * epsilon(1.0_dp) * 12.0_dp / (h * h)
        print '(a,i0,4(1x,es24.16e3))', ' DAVIDSON_GEN pair ', i, lambda(i), resid(i), own, exact(i)
        call check('davidson_gen: lambda_i within the residual bound of 6 (1 - c_i) / (h^2 (2 + c_i))', abs(lambda(i) - exact(i)) <= bar)
    enddo

    call pc%destroy()
    call A%destroy()
    call B%destroy()
    if (fails > 0) then
        print *, 'davidson_gen_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'davidson_gen_test_hip: ok'

contains

! tridiag(off, diag, off) of order nn
subroutine tridiag(M, off, diag)
    type(hip_csr_matrix), intent(inout) :: M
    real(dp), intent(in) :: off, diag
    integer :: r
    e = 0
    do r = 1, nn
        ptr(r) = e + 1
        if (r > 1) call put(r - 1, off)
        call put(r, diag)
        if (r < nn) call put(r + 1, off)
    enddo
    ptr(nn + 1) = e + 1
    call M%init(nn, nn, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
end subroutine

subroutine put(col, z)
    integer, intent(in) :: col
    real(dp), intent(in) :: z
    e = e + 1
    node(e) = col
    val(e) = z
end subroutine

subroutine check(what, ok)
    character(len=*), intent(in) :: what
    logical, intent(in) :: ok
    if (ok) then
        print *, 'ok    ', what
    else
        print *, 'FAILED ', what
        fails = fails + 1
    endif
end subroutine

end program davidson_gen_test_hip
