!==========================================================================!
! davidson_test_hip: the smallest eigenpairs through the stand-alone host   !
! layer.  The 5-point Laplacian of the 127 x 127 grid (eigenvalues          !
! 4 - 2 cos(i pi / 128) - 2 cos(j pi / 128), double for i /= j),            !
! hip_davidson for 4 pairs at the small end with ncv = 20 and tol = 1e-8    !
! from the default start vector, three times.  With hip_multigrid (the 2:1  !
! interpolations of mg_test_hip, V(1,1), omega = 0.8): the four smallest    !
! eigenpairs, the double eigenvalue twice, in about thirty steps.  With     !
! hip_jacobi() and without a preconditioner the search space is a Krylov    !
! space (this diagonal is constant), which holds one vector of every        !
! eigenspace: a double eigenvalue is reported once, as hip_eigsh reports    !
! it, and the steps are counted in hundreds.  Prints                        !
! every eigenvalue with the residual norm the library reports, the one this !
! program forms itself with A%matvec, and |v|_2, at full precision:         !
! tests/test_gpu_davidson.py reads them.                                    !
!==========================================================================!
program davidson_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx = 127, nn = nx * nx, k = 4, maxlev = 16
    real(dp), parameter :: pi = 3.14159265358979323846264338327950288_dp
    type(hip_csr_matrix), target :: A
    type(hip_csr_matrix), target :: P(maxlev)
    type(hip_matrix_pointer), allocatable :: Pp(:)
    type(hip_linear_solver), pointer :: pc, mg
    real(dp), allocatable :: V(:,:), q(:), val(:)
    integer, allocatable :: ptr(:), node(:)
    real(dp) :: exact(4, 4)
    integer :: i, j, r, e, fails, nlev, gx, l

    fails = 0
    call hip_check(sgm_init(0_c_int))
    allocate(V(nn, k), q(nn), val(5 * nn), ptr(nn + 1), node(5 * nn))
    e = 0
    do j = 1, nx
        do i = 1, nx
            r = (j - 1) * nx + i
            ptr(r) = e + 1
            if (j > 1) call put(r - nx, -1.0_dp)
            if (i > 1) call put(r - 1, -1.0_dp)
            call put(r, 4.0_dp)
            if (i < nx) call put(r + 1, -1.0_dp)
            if (j < nx) call put(r + nx, -1.0_dp)
        enddo
    enddo
    ptr(nn + 1) = e + 1
    call A%init(nn, nn, ptr, node(1:e))
    A%val = val(1:e)
    A%values_dirty = .true.
    do j = 1, 4
        do i = 1, 4
            exact(i, j) = 4.0_dp - 2.0_dp * cos(real(i, dp) * pi / 128.0_dp) - 2.0_dp * cos(real(j, dp) * pi / 128.0_dp)
        enddo
    enddo

    nlev = 0
    gx = nx
    do while (gx >= 5)
        nlev = nlev + 1
        call interp2d(P(nlev), gx, gx)
        gx = (gx + 1) / 2
    enddo
    allocate(Pp(nlev))
    do l = 1, nlev
        Pp(l)%mat => P(l)
    enddo
    mg => hip_multigrid(Pp, omega = 0.8_dp, nu_pre = 1, nu_post = 1, coarse_sweeps = 8)
    call mg%setup(A)
    call run('vcycle', mg)
    pc => hip_jacobi()
    call pc%setup(A)
    call run('jacobi', pc)
    call run('none')

    call mg%destroy()
    call pc%destroy()
    do l = 1, nlev
        call P(l)%destroy()
    enddo
    call A%destroy()
    if (fails > 0) then
        print *, 'davidson_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'davidson_test_hip: ok'

contains

subroutine run(label, m)
    character(len=*), intent(in) :: label
    type(hip_linear_solver), intent(in), optional :: m
    real(dp) :: lambda(k), resid(k), own, sorted(16)
    integer :: steps, products, applies, restarts, found, p, ia, ic
    logical :: converged
    if (present(m)) then
        call hip_davidson(A, k, lambda, pc=m, V=V, resid=resid, ncv=20, tol=1.0e-8_dp, max_steps=20000, steps=steps, &
            & products=products, applies=applies, restarts=restarts, found=found, converged=converged)
    else
        call hip_davidson(A, k, lambda, V=V, resid=resid, ncv=20, tol=1.0e-8_dp, max_steps=20000, steps=steps, &
            & products=products, applies=applies, restarts=restarts, found=found, converged=converged)
    endif
    call check('davidson ' // label // ': converged with 4 pairs', converged .and. found == k)
    call check('davidson ' // label // ': products = 1 + steps + pairs', products == 1 + steps + k)
    print '(a,a,a,i0,a,i0,a,i0,a,i0)', ' DAVIDSON ', label, ' steps ', steps, ' products ', products, ' applies ', applies, &
        & ' restarts ', restarts
    do p = 1, k
        call A%matvec(V(:, p), q)
        own = sqrt(sum((q - lambda(p) * V(:, p))**2))
        print '(a,a,a,i0,4(1x,es24.16e3))', ' DAVIDSON ', label, ' pair ', p, lambda(p), resid(p), own, sqrt(sum(V(:, p)**2))
        call check('davidson ' // label // ': within 1e-7 of an eigenvalue 4 - 2 cos(i pi / 128) - 2 cos(j pi / 128), i, j <= 4', &
            & minval(abs(lambda(p) - exact)) <= 1.0e-7_dp)
    enddo
    call check('davidson ' // label // ': the first is the smallest eigenvalue', abs(lambda(1) - exact(1, 1)) <= 1.0e-7_dp)
    if (label == 'vcycle') then
        ! the four smallest WITH multiplicity: the analytic values in ascending order (insertion sort of the 16)
        sorted = reshape(exact, [16])
        do ia = 2, 16
            own = sorted(ia)
            ic = ia - 1
            do while (ic >= 1)
                if (sorted(ic) <= own) exit
                sorted(ic + 1) = sorted(ic)
                ic = ic - 1
            enddo
            sorted(ic + 1) = own
        enddo
        call check('davidson vcycle: the four smallest eigenvalues, the double one twice', &
            & maxval(abs(lambda - sorted(1:k))) <= 1.0e-7_dp)
        call check('davidson vcycle: at most 40 steps', steps <= 40)
    endif
end subroutine

! the 2:1 linear interpolation from the coarse grid (the fine points of even i and j, 0-based) to an nx x ny grid
subroutine interp2d(M, nx, ny)
    type(hip_csr_matrix), intent(inout) :: M
    integer, intent(in) :: nx, ny
    integer :: ptr(nx * ny + 1), k, i, j, e, cx, cy, ii(2), jj(2), a, c
    real(dp) :: wi, wj
    integer, allocatable :: node(:)
    real(dp), allocatable :: val(:)
    cx = (nx + 1) / 2; cy = (ny + 1) / 2
    allocate(node(4 * nx * ny), val(4 * nx * ny))
    e = 0
    do k = 1, nx * ny
        i = mod(k - 1, nx); j = (k - 1) / nx
        ptr(k) = e + 1
        call along(i, cx, ii, wi)
        call along(j, cy, jj, wj)
        do a = 1, 2
            do c = 1, 2
                if (jj(a) >= 0 .and. ii(c) >= 0) then
                    e = e + 1
                    node(e) = jj(a) * cx + ii(c) + 1
                    val(e) = wi * wj
                endif
            enddo
        enddo
    enddo
    ptr(nx * ny + 1) = e + 1
    call M%init(nx * ny, cx * cy, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
end subroutine

subroutine along(t, c, idx, w)
    integer, intent(in) :: t, c
    integer, intent(out) :: idx(2)
    real(dp), intent(out) :: w
    idx(1) = t / 2
    idx(2) = -1
    w = 1.0_dp
    if (mod(t, 2) == 1) then
        w = 0.5_dp
        if (t / 2 + 1 < c) idx(2) = t / 2 + 1
    endif
end subroutine

subroutine put(c, z)
    integer, intent(in) :: c
    real(dp), intent(in) :: z
    e = e + 1
    node(e) = c
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

end program davidson_test_hip
